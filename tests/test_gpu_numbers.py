"""GPU: the device's number conversions against an arbiter that neither this project nor glibc wrote -- CPython's float(str),
repr(float) and int, through tests/number_cases.py (proved and counted on the CPU by tests/test_number_cases.py).

  text -> tape   the value and tag words of the fetched tape against the arbiter's bits / integers / kind / flag, compared
                 directly; the oracle comparison of test_gpu_parse.check runs on the same documents as well
  rejects        texts that round to +-Inf: a stage-2 error alone and in the middle of a long array, and the accepted text
                 one digit lower parses to the arbiter's bits on the same context right after
  tie-breaks     more than 3 x 4096 numbers that all take the big-integer path (k_bignum walks its queue 4096 at a time),
                 spread over an ordinary array and as the only content
  tape -> text   MarshalJSON of the arrays and the StringCvt column of the records against go_format of the arbiter's double
  conversions    extract_path FLOAT / INT / UINT and count_where_path EQ_* against column_walk.convert fed with the arbiter's
                 words (not the oracle's tape)
and the big ND document once more on a context that splits it into shards.  Strings stay out of these documents, so one copy
mode is enough.  A failure names the family, the text (first 60 bytes), and got / want as hex."""
import functools
import os
import random

import numpy as np
import pytest

import column_walk as CW
import number_cases as N
from test_gpu_parse import check, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

FAMILIES = N.FAMILIES
KINDS = (CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT)


# ---- the arbiter's side, computed once -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases(name):
    """[(family, text, expected)] of the accepted texts of a family; "all": of every family"""
    if name == "all":
        return [c for f in FAMILIES for c in cases(f)]
    return [(name, t, e) for t, e in N.accepted(N.families()[name])]


@functools.lru_cache(maxsize=None)
def want_words(name):
    return np.array([N.words(e) for _, _, e in cases(name)], dtype=np.uint64).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def want_texts(name):
    """what appendFloat / FormatInt / FormatUint print for the arbiter's values"""
    if name == "all":
        return [t for f in FAMILIES for t in want_texts(f)]
    return [N.go_format(N.bits2f(e[1])) if e[0] == "d" else str(e[1]) for _, _, e in cases(name)]


def array_doc(cs):
    return ("[" + ",".join(t for _, t, _ in cs) + "]").encode()


def nd_doc(cs):
    return "\n".join('{"v":%s}' % t for _, t, _ in cs).encode()


def array_words(tape, n):
    """root, '[', n x (tag, value), ']', root"""
    assert len(tape) == 2 * n + 4, (len(tape), n)
    assert int(tape[1]) >> 56 == ord("[") and int(tape[-2]) >> 56 == ord("]")
    return np.asarray(tape[2:2 + 2 * n]).reshape(n, 2)


def nd_words(tape, n):
    """per record: root, '{', the key (two words), (tag, value), '}', root"""
    assert len(tape) == 8 * n, (len(tape), n)
    rec = np.asarray(tape).reshape(n, 8)
    assert np.all(rec[:, 1] >> np.uint64(56) == ord("{")) and np.all(rec[:, 2] >> np.uint64(56) == ord('"'))
    return rec[:, 4:6]


def assert_words(what, cs, got, want):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        k = int(bad[0])
        fam, text, _ = cs[k]
        raise AssertionError("%s: %d of %d numbers differ; first: family %s, text %s, got %016x %016x, want %016x %016x" % (
            what, len(bad), len(cs), fam, text[:60], int(got[k, 0]), int(got[k, 1]), int(want[k, 0]), int(want[k, 1])))


def assert_texts(what, cs, got, want):
    assert len(got) == len(want) == len(cs), (what, len(got), len(want), len(cs))
    if got != want:
        k = next(i for i in range(len(want)) if got[i] != want[i])
        fam, text, e = cs[k]
        raise AssertionError("%s: family %s, text %s (value %016x): got %r, want %r" % (what, fam, text[:60], N.words(e)[1], got[k], want[k]))
    for (fam, text, e), g in zip(cs, got):  # and the text leads back to the same double
        if e[0] == "d":
            assert N.f2bits(float(g)) == e[1], "%s: family %s, text %s: %r reads back as %016x, want %016x" % (
                what, fam, text[:60], g, N.f2bits(float(g)), e[1])


def marshalled_numbers(ctx):
    out = ctx.marshal_json()
    assert out[:1] == b"[" and out[-1:] == b"]", out[:40]
    return out[1:-1].decode().split(",")


def cvt_texts(ctx, n):
    off, data, st = ctx.extract_path_strings((b"v",), cvt=True)
    assert len(st) == n and np.all(st == CW.COL_OK)
    off = off.tolist()
    return [data[off[k]:off[k + 1]].decode() for k in range(n)]


class _Element:  # what column_walk.convert reads: the tag word and the value word of one number
    def __init__(self, words):
        self.t = words


@functools.lru_cache(maxsize=None)
def want_column(name, kind):
    """Iter.Float / Int / Uint on the arbiter's words -> (value bits, statuses)"""
    vals, sts = [], []
    for tag, val in want_words(name).tolist():
        st, v = CW.convert(_Element((tag, val)), 0, kind)
        vals.append(v)
        sts.append(st)
    return np.array(vals, dtype=np.uint64), np.array(sts, dtype=np.uint8)


def assert_columns(what, ctx, name):
    cs = cases(name)
    for kind in KINDS:
        vals, st = ctx.extract_path((b"v",), kind)
        want_v, want_s = want_column(name, kind)
        assert len(st) == len(cs), (what, kind, len(st), len(cs))
        bad = np.nonzero((st != want_s) | (vals.view(np.uint64) != want_v))[0]
        if len(bad):
            k = int(bad[0])
            raise AssertionError("%s kind %d: %d records differ; first: family %s, text %s, got status %d value %016x, want %d %016x" % (
                what, kind, len(bad), cs[k][0], cs[k][1][:60], int(st[k]), int(vals.view(np.uint64)[k]), int(want_s[k]), int(want_v[k])))


# ---- text -> tape, tape -> text ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES)
def test_family_as_an_array(ctx, name):
    cs = cases(name)
    doc = array_doc(cs)
    pj = ctx.parse(doc)
    assert_words("array of " + name, cs, array_words(pj.Tape, len(cs)), want_words(name))
    for kf in (False, True):
        ctx.parse(doc, key_flags=kf)
        assert_texts("MarshalJSON of %s (key_flags %s)" % (name, kf), cs, marshalled_numbers(ctx), want_texts(name))
    check(ctx, doc, False, "array of " + name)


def test_all_families_as_one_array(ctx):
    cs = cases("all")
    doc = array_doc(cs)
    assert len(doc) > (16 << 20)  # far beyond the small-document path, several stage-2 tiles
    pj = ctx.parse(doc)
    assert_words("one array", cs, array_words(pj.Tape, len(cs)), want_words("all"))
    for kf in (False, True):
        ctx.parse(doc, key_flags=kf)
        assert_texts("MarshalJSON of one array (key_flags %s)" % kf, cs, marshalled_numbers(ctx), want_texts("all"))
    check(ctx, doc, False, "one array")


def test_all_families_as_records(ctx):
    cs = cases("all")
    doc = nd_doc(cs)
    pj = ctx.parse(doc, ndjson=True)
    assert_words("records", cs, nd_words(pj.Tape, len(cs)), want_words("all"))
    assert_texts("StringCvt of records", cs, cvt_texts(ctx, len(cs)), want_texts("all"))
    assert_columns("records", ctx, "all")
    # comparisons: a few dozen distinct values around the edges of the conversions, counted in Python on the arbiter's columns
    ops = {CW.COL_FLOAT: ctx.OP_EQ_FLOAT, CW.COL_INT: ctx.OP_EQ_INT, CW.COL_UINT: ctx.OP_EQ_UINT}
    rnd = random.Random(5)
    for kind, op in ops.items():
        vals, st = want_column("all", kind)
        ok = vals[st == CW.COL_OK]
        if kind == CW.COL_FLOAT:
            typed = ok.view(np.float64)
            probes = [0.0, -0.0, 1.0, 2.0 ** 63, 2.0 ** 64, -(2.0 ** 63), 5e-324, 1.7976931348623157e308, 9007199254740992.0, 1e23, 0.1, 1e22]
        elif kind == CW.COL_INT:
            typed = ok.view(np.int64)
            probes = [0, 1, -1, 2 ** 63 - 1, -(2 ** 63), 10 ** 18, -(10 ** 18), 9007199254740993, 2 ** 53]
        else:
            typed = ok
            probes = [0, 1, 2 ** 63, 2 ** 64 - 1, 2 ** 63 - 1, 10 ** 19, 2 ** 64 - 2, 9007199254740993]
        probes += [typed[rnd.randrange(len(typed))].item() for _ in range(8)]
        for v in probes:
            want = int((typed == typed.dtype.type(v)).sum())  # (doubles compare as doubles: -0.0 == 0.0)
            got = ctx.count_where_path((b"v",), op, v)
            assert got == want, ("count_where_path", kind, v, got, want)
    check(ctx, doc, True, "records")


def test_records_on_a_context_that_shards():
    import sjhip
    cs = cases("all")
    doc = nd_doc(cs)
    os.environ["SJHIP_ND_LIMIT_BYTES"] = str(2 << 20)
    os.environ["SJHIP_ND_SHARD_BYTES"] = str(1 << 20)
    try:
        many = sjhip.Context(0)
        pj = many.parse(doc, ndjson=True)
    finally:
        del os.environ["SJHIP_ND_LIMIT_BYTES"], os.environ["SJHIP_ND_SHARD_BYTES"]
    try:
        assert_words("sharded records", cs, nd_words(pj.Tape, len(cs)), want_words("all"))
        assert_texts("StringCvt of sharded records", cs, cvt_texts(many, len(cs)), want_texts("all"))
        assert_columns("sharded records", many, "all")
    finally:
        many.close()


# ---- rejects --------------------------------------------------------------------------------------------------------------------
def test_rejects_and_their_accepted_neighbours(ctx):
    import sjhip
    pairs = N.reject_pairs()
    assert len(pairs) >= 20
    around = cases("random_fill")[:3000]
    half = len(around) // 2
    for bad, good in pairs:
        e = N.expect(good)
        assert N.expect(bad) == "reject" and e != "reject"
        want = np.array([N.words(e)], dtype=np.uint64)
        for what, before, after in (("alone", [], []), ("in a long array", around[:half], around[half:])):
            with pytest.raises(sjhip.ParseError) as err:
                ctx.parse(array_doc(before + [("top", bad, None)] + after))
            assert err.value.code == 2, (what, bad[:60], err.value.code)  # "Bad parsing while executing stage 2"
            cs = before + [("top", good, e)] + after
            pj = ctx.parse(array_doc(cs))
            got = array_words(pj.Tape, len(cs))
            assert_words("neighbour of a reject, " + what, [cs[len(before)]], got[len(before):len(before) + 1], want)
        check(ctx, array_doc([("top", bad, None)]), False, "reject")


# ---- the queue of the big-integer kernel ------------------------------------------------------------------------------------
def number_words(tape):
    """(tag, value) of every number of a tape, in order (strings take two words like numbers, everything else one)"""
    out, i, t = [], 0, np.asarray(tape).tolist()
    while i < len(t):
        tag = t[i] >> 56
        if tag in (0x6C, 0x75, 0x64):  # l u d
            out.append((t[i], t[i + 1]))
            i += 2
        else:
            i += 2 if tag == 0x22 else 1
    return np.array(out, dtype=np.uint64).reshape(-1, 2)


def test_tie_break_density(ctx):
    big = cases("tiebreak")
    assert len(big) >= 3 * 4096 + 1  # (that all of them take the big-integer path is asserted in test_number_cases.py)
    fill = cases("random_fill")
    rnd = random.Random(17)
    parts, cs, at = [], [], 0
    for c in big:  # an ordinary array around them: records with strings, nested arrays, short numbers
        k = rnd.randrange(3, 9)
        inner = fill[at:at + k]
        at += k
        parts.append('{"id":"r%d","tags":["a","b\\n"],"x":[%s],"ok":true,"big":%s,"n":null}' % (len(cs), ",".join(t for _, t, _ in inner), c[1]))
        cs += inner + [c]
    doc = ("[" + ",\n".join(parts) + "]").encode()
    assert len(doc) > (6 << 20)
    want = np.array([N.words(e) for _, _, e in cs], dtype=np.uint64).reshape(-1, 2)
    pj = ctx.parse(doc)
    assert_words("tie-breaks spread over records", cs, number_words(pj.Tape), want)
    check(ctx, doc, False, "tie-breaks spread over records")
    doc = array_doc(big)  # and as the only content: every number of every tile goes to the queue
    pj = ctx.parse(doc)
    assert_words("tie-breaks alone", big, array_words(pj.Tape, len(big)), want_words("tiebreak"))
    nd = nd_doc(big)
    pj = ctx.parse(nd, ndjson=True)
    assert_words("tie-breaks as records", big, nd_words(pj.Tape, len(big)), want_words("tiebreak"))
