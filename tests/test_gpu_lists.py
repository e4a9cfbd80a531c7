"""GPU: list columns at a path (sjhip_extract_path_list / sjhip_extract_path_list_strings and their fetches) against the restated
array conversions of tests/list_walk.py over the oracle's parse -- list offsets, values as bits, string offsets, bytes and
statuses, bit for bit, in both copy modes: generated records, long and skewed arrays, the number texts of canada.json, twitter's
statuses, a sharded result against the same message parsed whole, the lifecycle of the list column, and the existing path queries
on the same paths."""
import json
import random
import re

import numpy as np
import pytest

import column_walk as CW
import fixtures
import list_walk as LW
import oracle_lib as O
import query_walk as Q
from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = (LW.COL_FLOAT, LW.COL_INT, LW.COL_UINT)
OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)


def oracle_walk(doc, nd, copy):
    ref = O.parse(doc, ndjson=nd, copy_strings=copy)
    assert ref.rc == 0
    return Q.Walk(ref.tape, ref.strings, doc[ref.msg_off:ref.msg_off + ref.msg_len])


def check_numbers(ctx, w, path, kinds=KINDS):
    seen = {}
    for kind in kinds:
        off, vals, st = ctx.extract_path_list(path, kind)
        want_o, want_v, want_s = LW.list_column(w, path, kind)
        assert np.array_equal(st, np.array(want_s, dtype=np.uint8)), (path, kind)
        assert off.dtype == np.uint64 and np.array_equal(off, np.array(want_o, dtype=np.uint64)), (path, kind)
        assert vals.dtype == ctx._COL_DTYPES[kind]
        assert np.array_equal(vals.view(np.uint64), np.array(want_v, dtype=np.uint64)), (path, kind)
        seen[kind] = set(want_s)
    return seen


def check_strings(ctx, w, path, cvts=(False, True)):
    seen = {}
    for cvt in cvts:
        off, soff, data, st = ctx.extract_path_list_strings(path, cvt=cvt)
        want_o, want_so, want_d, want_s = LW.list_string_column(w, path, cvt)
        assert np.array_equal(st, np.array(want_s, dtype=np.uint8)), (path, cvt)
        assert off.dtype == np.uint64 and np.array_equal(off, np.array(want_o, dtype=np.uint64)), (path, cvt)
        assert soff.dtype == np.uint64 and np.array_equal(soff, np.array(want_so, dtype=np.uint64)), (path, cvt)
        assert data == want_d, (path, cvt)
        seen["c" if cvt else "s"] = set(want_s)
    return seen


def check_doc(ctx, doc, nd, paths, copy):
    w = oracle_walk(doc, nd, copy)
    ctx.parse(doc, ndjson=nd, copy_strings=copy)
    seen = {}
    for path in paths:
        for k, s in {**check_numbers(ctx, w, path), **check_strings(ctx, w, path)}.items():
            seen.setdefault(k, set()).update(s)
    return w, seen


# ---- seeded generated records -------------------------------------------------------------------------------------------------
EDGES = ["9223372036854775808.0", "-9223372036854775808.0", "9223372036854777856.0", "-9223372036854777856.0", "18446744073709551616.0",
         "18446744073709555712.0", "-0.0", "-0", "0", "1e308", "-1e308", "4.9e-324", "2.2250738585072014e-308", "1e-7", "1e21",
         "123456.789e-3", "0.1000000000000000055511151231257827", "3.141592653589793238462643383279", "9223372036854775807",
         "9223372036854775808", "18446744073709551615", "-9223372036854775808", "-9223372036854775809", "-1", "1", "100"]
SAFE = ["0", "1", "7", "2.5", "100", "1e3", "9223372036854775807", "0.125", "4.9e-324", "-0.0", "9223372036854775808.0"]  # (fit every kind)
STRINGS = ['""', '"x"', '"HOND"', '"a\\"b\\\\c\\/d\\n\\t"', '"\\u00e9\\u4e2d\\ud83d\\ude00"', '"3"', '"true"', '"café é"']
STRINGS += ['"' + "a long string, " * 3 + '\\u00e9"']  # (longer than a lane copies alone)
LONG = '"' + "x" * 3000 + '\\n"'
KEYS = ['"a"', '"b"', '"c"', '""', '"\\u0061"', '"a\\"q"']  # (the fifth is "a" through an escape)


def rstring(rnd):
    return LONG if rnd.random() < 0.02 else rnd.choice(STRINGS)


def rarray(rnd):
    r = rnd.random()
    n = rnd.choice([0, 1, 2, 3, 5, 17, 40, 70, 130]) if rnd.random() < 0.8 else rnd.randint(0, 9)
    if r < 0.25:
        items = [rnd.choice(SAFE) for _ in range(n)]
    elif r < 0.45:
        items = [rnd.choice(EDGES) if rnd.random() < 0.2 else rnd.choice(SAFE) for _ in range(n)]
    elif r < 0.65:
        items = [rstring(rnd) for _ in range(n)]
    elif r < 0.8:  # scalars of every kind: AsStringCvt's ground
        items = [rstring(rnd) if rnd.random() < 0.3 else rnd.choice(SAFE + ["true", "false", "null", "-5", "1.5e300"]) for _ in range(n)]
    else:  # one odd element somewhere in numbers or strings
        base = SAFE if rnd.random() < 0.5 else STRINGS
        items = [rnd.choice(base) if base is SAFE else rstring(rnd) for _ in range(max(n, 1))]
        items[rnd.randrange(len(items))] = rnd.choice(["null", "true", "[1]", "{}", '{"a":[1]}', "[]", '"s"', "-1", "1e300", "2"])
    return "[" + ",".join(items) + "]"


def rvalue(rnd, depth):
    r = rnd.random()
    if r < 0.55:
        return rarray(rnd)
    if r < 0.62:
        return rnd.choice(["null", "true", "5", '"s"', "2.5"])
    if depth < 3 and r < 0.95:
        return robj(rnd, depth + 1)
    return "null"


def robj(rnd, depth):
    return "{" + ",".join("%s:%s" % (rnd.choice(KEYS), rvalue(rnd, depth)) for _ in range(rnd.randint(0, 4))) + "}"


def random_nd(seed, n):
    rnd = random.Random(seed)
    return "\n".join(robj(rnd, 0) if rnd.random() < 0.92 else rarray(rnd) for _ in range(n)).encode()  # (some roots are arrays)


RANDOM_PATHS = [(b"a",), (b"b",), (b"",), (b'a"q',), (b"a", b"b"), (b"b", b"a"), (b"a", b""), (b"a", b"b", b"c"), (b"c", b"c", b"a")]


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
def test_random_records(ctx, copy):
    doc = random_nd(31, 2500)
    _, seen = check_doc(ctx, doc, True, RANDOM_PATHS, copy)
    # every status occurs for every kind (RANGE is an answer of AsInteger and AsUint64 alone: parsed_array.go has no other)
    for kind in (LW.COL_INT, LW.COL_UINT):
        assert seen[kind] == set(range(6)), (kind, seen[kind])
    for kind in (LW.COL_FLOAT, "s", "c"):
        assert seen[kind] == {OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL}, (kind, seen[kind])


# ---- long and skewed arrays ---------------------------------------------------------------------------------------------------
def test_long_and_skewed_arrays(ctx):
    rnd = random.Random(32)
    nums = [rnd.choice(SAFE) if rnd.random() < 0.3 else str(rnd.randint(0, 2 ** 62)) if rnd.random() < 0.6 else repr(rnd.uniform(0, 1e9))
            for _ in range(200003)]
    short = ['{"p":[%s],"t":["%s"]}' % (",".join(rnd.choice(SAFE) for _ in range(rnd.randint(0, 4))), "s" * rnd.randint(0, 40))
             for _ in range(3000)]
    long_ok = ",".join(rnd.choice(SAFE) for _ in range(1000))
    lines = short[:1500] + ['{"p":[%s],"t":[]}' % ",".join(nums)] + short[1500:] + [
        # the only bad element beyond the first wave step: TYPE, and RANGE for both integer kinds
        '{"p":[%s,"bad",%s]}' % (long_ok, long_ok),
        '{"p":[%s,1e300,%s]}' % (long_ok, long_ok),
        '{"p":[%s,null]}' % long_ok,
        # a one-word element followed by numbers: what lies behind it is read from shifted words and must not decide
        '{"p":[%s,true,%s]}' % (long_ok, ",".join(["1e300", "-1", "7"] * 200)),
        '{"p":[true,%s]}' % ",".join(["1e300", "-1"] * 300),
        # a RANGE in front of a TYPE in the same step, and the reverse
        '{"p":[%s,-1.5,"x",%s]}' % (long_ok, long_ok),
        '{"p":[%s,"x",-1.5,%s]}' % (long_ok, long_ok),
        # a long array of long strings, one with a number inside, one of empty strings
        '{"t":[%s]}' % ",".join('"%s\\n"' % (chr(97 + k % 26) * (33 + 37 * (k % 50))) for k in range(700)),
        '{"t":[%s,5,"x"]}' % ",".join('"%s"' % ("y" * (k % 90)) for k in range(300)),
        '{"t":[%s]}' % ",".join(['""'] * 500),
        # long arrays of every scalar for AsStringCvt
        '{"t":[%s]}' % ",".join(rnd.choice(SAFE + ["true", "false", "null", '"' + "z" * 200 + '"', '"q"', "-7", "1e-7"]) for _ in range(2000)),
        '{"t":[%s,[],1]}' % ",".join(["null"] * 900),
    ]
    doc = "\n".join(lines).encode()
    for copy in (True, False):
        w, seen = check_doc(ctx, doc, True, [(b"p",), (b"t",)], copy)
        assert RANGE in seen[LW.COL_INT] and TYPE in seen[LW.COL_FLOAT]
    off, vals, st = ctx.extract_path_list((b"p",), LW.COL_FLOAT)
    assert int((off[1:] - off[:-1]).max()) == 200003


# ---- real number texts --------------------------------------------------------------------------------------------------------
def test_canada_pairs(ctx):
    text = fixtures.load("canada").decode()
    pairs = re.findall(r"\[\s*(-?[0-9][0-9.eE+-]*)\s*,\s*(-?[0-9][0-9.eE+-]*)\s*\]", text)  # (the digits stay the fixture's)
    assert len(pairs) > 50000
    lines = ['{"p":[%s,%s]}' % p for p in pairs]
    lines.insert(len(lines) // 2, '{"p":[%s]}' % ",".join("%s,%s" % p for p in pairs))
    doc = "\n".join(lines).encode()
    for copy in (True, False):
        w = oracle_walk(doc, True, copy)
        ctx.parse(doc, ndjson=True, copy_strings=copy)
        seen = check_numbers(ctx, w, (b"p",))
        assert seen[LW.COL_FLOAT] == {OK} and RANGE in seen[LW.COL_UINT] <= {OK, RANGE}  # (the longitudes are negative)
        check_strings(ctx, w, (b"p",), cvts=(True,))
    off, vals, st = ctx.extract_path_list((b"p",), LW.COL_FLOAT)
    assert len(vals) == 4 * len(pairs) and vals[0] == float(pairs[0][0]) and vals[-1] == float(pairs[-1][1])


def test_twitter_statuses(ctx):
    statuses = json.loads(fixtures.load("twitter"))["statuses"]
    doc = "\n".join(json.dumps(s, ensure_ascii=False, separators=(",", ":")) for s in statuses).encode()
    paths = [(b"geo", b"coordinates"), (b"coordinates", b"coordinates"), (b"entities", b"hashtags"), (b"entities", b"urls")]
    for copy in (True, False):
        w, seen = check_doc(ctx, doc, True, paths, copy)
    off, soff, data, st = ctx.extract_path_list_strings((b"entities", b"hashtags"))
    assert set(st.tolist()) == {OK, TYPE}  # (an empty list, or a list of objects)
    assert int(off[-1]) == 0 and data == b""


# ---- a sharded result ---------------------------------------------------------------------------------------------------------
def test_sharded_result_equals_whole():
    import sjhip
    park = fixtures.load("parking-citations")
    doc = random_nd(33, 1200) + b"\n" + park * 3 + random_nd(34, 1200) + b"\n" + park * 2
    assert len(doc) > (2 << 20)
    paths = [(b"a",), (b"b",), (b"a", b"b"), (b"Make",)]
    one = sjhip.Context(0)
    for copy in (True, False):
        one.parse(doc, ndjson=True, copy_strings=copy)
        want = {p: ([one.extract_path_list(p, k) for k in KINDS], [one.extract_path_list_strings(p, cvt=c) for c in (False, True)])
                for p in paths}
        with fixtures.nd_shard_limits(2 << 20, 1 << 20):
            many = sjhip.Context(0)
            many.parse(doc, ndjson=True, copy_strings=copy)
        w = oracle_walk(doc, True, copy)
        for p in paths:
            nums, strs = want[p]
            for k, (o1, v1, s1) in zip(KINDS, nums):
                o2, v2, s2 = many.extract_path_list(p, k)
                assert np.array_equal(o1, o2) and np.array_equal(v1.view(np.uint64), v2.view(np.uint64)) and np.array_equal(s1, s2), (p, k, copy)
            for cvt, (o1, so1, d1, s1) in zip((False, True), strs):
                o2, so2, d2, s2 = many.extract_path_list_strings(p, cvt=cvt)
                assert np.array_equal(o1, o2) and np.array_equal(so1, so2) and d1 == d2 and np.array_equal(s1, s2), (p, cvt, copy)
            check_numbers(many, w, p, kinds=(LW.COL_INT,))
            check_strings(many, w, p, cvts=(True,))
        many.close()
    one.close()


# ---- the lifecycle ------------------------------------------------------------------------------------------------------------
def test_lifecycle(ctx):
    import sjhip
    doc = b'{"s":["abc","de"],"n":[1,2.5]}\n{"s":[],"n":[3]}\n{"n":null,"s":["f"]}'
    # fetch without a list column
    fresh = sjhip.Context(0)
    fresh.parse(doc, ndjson=True)
    held = fresh.device_bytes()
    for fetch in (lambda: fresh.fetch_path_list(3, 3, LW.COL_FLOAT), lambda: fresh.fetch_path_list_strings(3, 3, 6)):
        with pytest.raises(sjhip.ParseError) as e:
            fetch()
        assert e.value.code == 5 and "no list column" in str(e.value)
    # fetch of the wrong kind
    assert fresh.extract_path_list((b"n",), LW.COL_FLOAT, fetch=False) == (3, 3)
    with pytest.raises(sjhip.ParseError) as e:
        fresh.fetch_path_list_strings(3, 3, 0)
    assert e.value.code == 5 and "no list column" in str(e.value)
    off, vals, st = fresh.fetch_path_list(3, 3, LW.COL_FLOAT)
    assert off.tolist() == [0, 2, 3, 3] and vals.tolist() == [1.0, 2.5, 3.0] and st.tolist() == [OK, OK, NULL]
    assert fresh.extract_path_list_strings((b"s",), fetch=False) == (3, 3, 6)
    with pytest.raises(sjhip.ParseError) as e:
        fresh.fetch_path_list(3, 3, LW.COL_FLOAT)
    assert e.value.code == 5 and "no list column" in str(e.value)
    off, soff, data, st = fresh.fetch_path_list_strings(3, 3, 6)
    assert off.tolist() == [0, 2, 2, 3] and soff.tolist() == [0, 3, 5, 6] and data == b"abcdef" and st.tolist() == [OK, OK, OK]
    # there is no bool conversion of arrays
    with pytest.raises(sjhip.ParseError) as e:
        fresh.extract_path_list((b"n",), fresh.COL_BOOL)
    assert e.value.code == 5
    # the arena is counted and trimmed
    assert fresh.device_bytes() > held
    fresh.trim()
    assert fresh.device_bytes() < held
    with pytest.raises(sjhip.ParseError):
        fresh.fetch_path_list_strings(3, 3, 6)
    fresh.close()
    # a parse in between drops the column; the next extraction holds no stale elements
    ctx.parse(doc, ndjson=True)
    nr, ne = ctx.extract_path_list((b"n",), LW.COL_INT, fetch=False)
    ctx.parse(b'{"n":[9]}\n{"n":[]}', ndjson=True)
    with pytest.raises(sjhip.ParseError):
        ctx.fetch_path_list(nr, ne, LW.COL_INT)
    off, vals, st = ctx.extract_path_list((b"n",), LW.COL_INT)
    assert off.tolist() == [0, 1, 1] and vals.tolist() == [9] and st.tolist() == [OK, OK]
    # list and string columns, the other queries, MarshalJSON, filter and serialize in between leave each other's columns intact
    rnd = random.Random(35)
    lines = ['{"Make":"%s","tags":[%s],"xs":[%s]}' % (rnd.choice(["HOND", "TOYT", "x" * 50]), ",".join(rnd.choice(STRINGS) for _ in range(rnd.randint(0, 5))),
                                                     ",".join(rnd.choice(SAFE) for _ in range(rnd.randint(0, 30)))) for _ in range(3000)]
    big = "\n".join(lines).encode()
    ctx.parse(big, ndjson=True, key_flags=True)
    w = oracle_walk(big, True, True)
    want_l = LW.list_string_column(w, (b"tags",), False)
    want_c = CW.string_column(w, (b"Make",), True)
    nr, ne, nb = ctx.extract_path_list_strings((b"tags",), fetch=False)
    cr, cb = ctx.extract_path_strings((b"Make",), cvt=True, fetch=False)
    ctx.marshal_json()
    ctx.filter_where(b"Make", b"HOND")
    ctx.serialize()
    ctx.find_path(b"xs")
    ctx.extract_path((b"Make",), CW.COL_INT)
    ctx.count_where_path((b"tags",), ctx.OP_EXISTS)
    off, soff, data, st = ctx.fetch_path_list_strings(nr, ne, nb)
    assert (off.tolist(), soff.tolist(), data, st.tolist()) == want_l
    nr, ne = ctx.extract_path_list((b"xs",), LW.COL_FLOAT, fetch=False)  # (a list column replaces a list column, not the string column)
    o2, d2, s2 = ctx.fetch_path_strings(cr, cb)
    assert (o2.tolist(), d2, s2.tolist()) == want_c
    ctx.extract_path_strings((b"Make",))
    off, vals, st = ctx.fetch_path_list(nr, ne, LW.COL_FLOAT)
    want_o, want_v, want_s = LW.list_column(w, (b"xs",), LW.COL_FLOAT)
    assert off.tolist() == want_o and vals.view(np.uint64).tolist() == want_v and st.tolist() == want_s
    # a column with no OK record, and a column of empty arrays
    ctx.parse(b'{"e":[]}\n{"e":[]}\n{"e":[]}', ndjson=True)
    for kind in KINDS:
        off, vals, st = ctx.extract_path_list((b"nope",), kind)
        assert off.tolist() == [0, 0, 0, 0] and len(vals) == 0 and st.tolist() == [NOT_FOUND] * 3
        off, vals, st = ctx.extract_path_list((b"e",), kind)
        assert off.tolist() == [0, 0, 0, 0] and len(vals) == 0 and st.tolist() == [OK] * 3
    for cvt in (False, True):
        off, soff, data, st = ctx.extract_path_list_strings((b"nope",), cvt=cvt)
        assert off.tolist() == [0, 0, 0, 0] and soff.tolist() == [0] and data == b"" and st.tolist() == [NOT_FOUND] * 3
        off, soff, data, st = ctx.extract_path_list_strings((b"e",), cvt=cvt)
        assert off.tolist() == [0, 0, 0, 0] and soff.tolist() == [0] and data == b"" and st.tolist() == [OK] * 3


def test_consistent_with_the_path_queries(ctx):
    doc = random_nd(36, 2000)
    for copy in (True, False):
        ctx.parse(doc, ndjson=True, copy_strings=copy)
        for path in RANDOM_PATHS:
            idx = ctx.find_path(*path)
            exists = ctx.count_where_path(path, ctx.OP_EXISTS)
            cols = [ctx.extract_path_list(path, k)[2] for k in KINDS] + [ctx.extract_path_list_strings(path, cvt=c)[3] for c in (False, True)]
            for st in cols:
                assert np.array_equal(st == NOT_FOUND, idx == Q.NOT_FOUND), path
                assert np.array_equal(st == NOT_OBJECT, idx == Q.NOT_OBJECT), path
                assert int(((st != NOT_FOUND) & (st != NOT_OBJECT)).sum()) == exists, path
                assert int((st == NULL).sum()) == ctx.count_where_path(path, ctx.OP_IS_NULL), path
