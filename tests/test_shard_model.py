"""CPU: the sharded ParseND on the host -- cuts, windows, bases and verdict (tests/shard_model.py) -- against the oracle's ParseND of
the whole message, for every document of the built family, every n in 1..8 and both copy modes: the windows of the Python model
equal those of the exported C++ rule (csrc/sj_host.h shard_windows), the verdict is the oracle's, and on success tape, Strings.B
and message window are the oracle's bit for bit; the same through sjhip.ndshard.parse_shard with host callbacks.
test_the_construction_holds asserts on the documents themselves that the stated seam is hit at the stated n.

Top-level scalars: the reference's ParseND rejects a scalar root (stage 2), so "scalar roots" is a failing document here and
"scalars in arrays" carries the scalar values behind a root."""
import numpy as np
import pytest

import oracle_lib as O
import shard_model as M

CASES = [(name, n) for name in M.DOCS for n in M.N_RANGE]
IDS = ["%s-%d" % (name.replace(" ", "_").replace(",", ""), n) for name, n in CASES]


@pytest.fixture(scope="module")
def refs():
    return {(name, copy): O.parse(doc, ndjson=True, copy_strings=copy) for name, doc in M.DOCS.items() for copy in (True, False)}


def test_expected_verdicts(refs):
    """what the issue of this family states about the whole message, by the oracle"""
    for (name, _), ref in refs.items():
        want = 0
        if "behind records" in name or "in front of records" in name or name in ("scalar roots", "stage 2 twice", "record broken at a newline"):
            want = 2
        if name in ("stage 2 first, stage 1 last", "string closed in the next shard"):
            want = 1
        assert ref.rc == want, name
    for name, w in M.BLANKS.items():  # the global trim removes them: the window starts behind them
        ref = refs["%s around the message" % name, False]
        assert (ref.msg_off, ref.msg_len) == (len(w), len(M.DOCS["%s around the message" % name]) - 2 * len(w))


@pytest.mark.parametrize("name,n", CASES, ids=IDS)
def test_windows_equal_the_cpp_rule(name, n):
    doc = M.DOCS[name]
    wins, g_off, g_len = M.windows(doc, n)
    cwins, cinner, c_off, c_len = M.cpp_windows(doc, n)
    assert (g_off, g_len) == (c_off, c_len)
    assert wins == cwins
    assert M.inner(wins) == cinner
    # ... and the cuts are ndshard.record_cuts', the windows ndshard.shard_windows'
    from sjhip import ndshard
    c = M.cuts(doc, n)
    assert ndshard.record_cuts(doc, n) == list(zip(c, c[1:]))
    assert ndshard.shard_windows(doc, n, g_off, g_len) == wins


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
@pytest.mark.parametrize("name,n", CASES, ids=IDS)
def test_merged_equals_oracle(refs, name, n, copy):
    doc, ref = M.DOCS[name], refs[name, copy]
    rc, tape, strings, g_off, g_len = M.merged(doc, n, copy)
    assert rc == ref.rc, (rc, ref.rc, M.window_bytes(doc, n))
    if rc == 0:
        assert (g_off, g_len) == (ref.msg_off, ref.msg_len)
        assert np.array_equal(tape, ref.tape)
        assert np.array_equal(strings, ref.strings)


class _Stop(Exception):
    pass


def _through_ndshard(doc, n, copy):
    """sjhip.ndshard.parse_shard for every rank in one process: the gather is a list that is filled rank by rank (every rank runs up
    to the exchange whose list is not full yet, then again) -> (code, tapes, strings)"""
    from sjhip import ndshard
    from sjhip.api import ParseError
    flags = 1 | (2 if copy else 0)

    def callbacks():
        state = {}

        def run(tb, sb, mb, fl):
            rc, t, s = M.replay(state["w"], fl, tb, sb, mb)
            if rc:
                raise ParseError("host replay rc %d" % rc, rc)
            return t, s

        def begin(window, inner=False):
            state["w"] = window
            t, s = run(0, 0, 0, flags | (M.FLAG_INNER if inner else 0))
            return len(t), len(s)

        return (lambda b: M.trim_space(b)), begin, (lambda tb, sb, mb: run(tb, sb, mb, flags))

    boxes = [[None] * n, [None] * n]
    out = [None] * n
    for have in (0, 1, 2):  # exchanges whose list is full
        for r in range(n):
            calls = [0]

            def gather(vals, r=r, calls=calls):
                k = calls[0]
                calls[0] += 1
                if k < have:
                    return boxes[k]
                boxes[k][r] = tuple(int(v) for v in vals)
                raise _Stop()
            trim, begin, finish = callbacks()
            try:
                out[r] = ndshard.parse_shard(doc, r, n, trim, begin, finish, gather, copy)
            except _Stop:
                pass
            except ndshard.ShardError as e:
                out[r] = e.code
        if any(isinstance(o, int) for o in out):
            assert all(o == out[0] for o in out), out  # every rank raises the same error
            return out[0], None, None
    for r, (t, s, tb, sb) in enumerate(out):
        assert (tb, sb) == (sum(len(o[0]) for o in out[:r]), sum(len(o[1]) for o in out[:r]))
    return 0, np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "nocopy"])
@pytest.mark.parametrize("name,n", CASES, ids=IDS)
def test_through_ndshard_equals_oracle(refs, name, n, copy):
    doc, ref = M.DOCS[name], refs[name, copy]
    if ref.msg_len == 0:
        pytest.fail("the family holds no blank document")
    rc, tape, strings = _through_ndshard(doc, n, copy)
    assert rc == ref.rc, (rc, ref.rc, M.window_bytes(doc, n))
    if rc == 0:
        assert np.array_equal(tape, ref.tape)
        assert np.array_equal(strings, ref.strings)


# ---- the construction ---------------------------------------------------------------------------------------------------------
def _word_kinds(tape):
    """index words (roots, brackets) / string words / value words of a tape"""
    tags = (tape >> np.uint64(56)).astype(np.uint8)
    raw = np.zeros(len(tape), dtype=bool)
    k = 0
    while k < len(tape):  # the word behind a string, an integer or a float is a value
        if tags[k] in b'"lud':
            raw[k + 1] = True
            k += 2
        else:
            k += 1
    return tags, raw


def test_the_construction_holds():
    D = M.DOCS
    t2 = lambda name: (D[name], M.targets(D[name], 2)[0])
    doc, t = t2("target on a newline")
    assert doc[t:t + 1] == b"\n" and M.cuts(doc, 2)[1] == t + 1
    doc, t = t2("target before a newline")
    assert doc[t + 1:t + 2] == b"\n" and doc[t:t + 1] != b"\n" and M.cuts(doc, 2)[1] == t + 2
    doc, t = t2("target after a newline")
    assert doc[t - 1:t] == b"\n" and doc[t:t + 1] == b"{" and M.cuts(doc, 2)[1] == doc.index(b"\n", t) + 1  # the NEXT newline
    doc, t = t2("target on the CR of CRLF")
    assert doc[t:t + 2] == b"\r\n" and M.cuts(doc, 2)[1] == t + 2 and M.window_bytes(doc, 2)[0].endswith(b'"}')
    doc, t = t2("target in blank lines")
    assert doc[t - 2:t + 3] == b"\n" * 5 and M.cuts(doc, 2)[1] == t + 1 and M.window_bytes(doc, 2)[1].startswith(b"{")
    doc, t = t2("target in an escaped n")
    assert doc[t:t + 2] == b"\\n" and doc[:t].count(b'"') % 2 == 1 and M.cuts(doc, 2)[1] == doc.index(b"\n") + 1
    # a record longer than len / n: every target lies inside it, the cuts behind it are found from the previous cut (one per newline:
    # the blank lines give empty shards in the middle), and when the newlines run out the cuts share len (empty shards at the end)
    doc = D["long record"]
    c = M.cuts(doc, 8)
    w = M.window_bytes(doc, 8)
    assert 200 > len(doc) // 8 and all(13 < t < 213 for t in M.targets(doc, 8)) and c[1] == 214
    assert c[2:5] == [215, 216, 229] and c[5] == c[6] == c[7] == c[8] == len(doc)
    assert [bool(x) for x in w] == [True, False, False, True, True, False, False, False], w
    assert w[0].count(b"\n") == 1
    doc = D["one record"]
    assert b"\n" not in doc and all([bool(x) for x in M.window_bytes(doc, n)] == [True] + [False] * (n - 1) for n in M.N_RANGE)
    assert M.windows(doc, 3)[0][0] == (2, len(doc) - 1)
    doc = D["two records"]
    assert all(sum(bool(x) for x in M.window_bytes(doc, n)) == 2 for n in range(2, 9)) and doc.count(b"\n") + 1 < 3
    assert [bool(x) for x in M.window_bytes(doc, 8)] == [True, True] + [False] * 6
    # edges: the byte stays at the end (the start) of some shard for EVERY n -- 4 records, so n = 4 has each record alone -- and n = 2, 3
    # leave some of them inside a shard
    for name, b in M.BLANKS.items():
        for n in range(2, 9):
            assert any(x.endswith(b) for x in M.window_bytes(D["%s behind records" % name], n)), (name, n)
            assert any(x.startswith(b) for x in M.window_bytes(D["%s in front of records" % name], n)), (name, n)
        assert [x.endswith(b) for x in M.window_bytes(D["%s behind records" % name], 4)] == [True, True, True, False]
        assert [x.startswith(b) for x in M.window_bytes(D["%s in front of records" % name], 4)] == [False, True, True, False]
        assert any(b + b"\n{" in x for x in M.window_bytes(D["%s behind records" % name], 2))
        doc = D["%s around the message" % name]
        for n in M.N_RANGE:
            wins, g_off, g_len = M.windows(doc, n)
            assert g_off == len(b) and wins[0][0] == g_off and max(e for a, e in wins if e > a) == len(doc) - len(b)
        assert sum(bool(x) for x in M.window_bytes(doc, 2)) == 2   # a later shard's strings count from behind the blank
    doc = D["space, tab and CR runs"]
    for n in M.N_RANGE:
        for x in M.window_bytes(doc, n):
            assert x == b"" or (x[:1] == b"{" and x[-1:] == b"}")
    assert sum(bool(x) for x in M.window_bytes(doc, 3)) == 3
    # rebased: a later shard begins with each of these
    def begins(name, prefix):
        return any(x.startswith(prefix) for n in range(2, 9) for x in M.window_bytes(D[name], n)[1:])
    for p in (b"1", b'"s"', b"true"):
        assert begins("scalar roots", p), p
    for p in (b"[1]", b'["s"]', b"[true]", b"[1.5]"):
        assert begins("scalars in arrays", p), p
    for p in (b"{}", b"[]", b"[[]]"):
        assert begins("empty containers", p), p
    ref = O.parse(D["empty containers"], ndjson=True)
    tags, raw = _word_kinds(ref.tape)
    assert not raw.any() and set(tags.tolist()) <= set(b"r{}[]")   # index words only
    assert begins("nested 12 deep", b"[" * 12)
    assert begins("strings", b'{"k3":"plain3","e":"q\\"3')
    doc = D["numbers like tags"]
    ref = O.parse(doc, ndjson=True)
    tags, raw = _word_kinds(ref.tape)
    tops = set((ref.tape[raw] >> np.uint64(56)).astype(np.uint8).tolist())
    assert {0x7B, 0x5B, 0x72, 0x22} <= tops and {0x7A, 0x5A, 0x71, 0x21} <= tops, tops  # the values and the neighbours below
    assert ref.tape[raw].tolist().count(0x2200000000000003) == 4 and ref.tape[raw].tolist().count(0x7B0F000000000000) == 4
    assert all(begins("numbers like tags", b"[%d," % (v - 1)) for v in (6557241057451442176, 8214565720323784704, 2449958197289549824))
    # a shard without any string in front of one with strings; a shard with nothing but strings in front of the rest
    w = M.window_bytes(D["no strings, then strings"], 2)
    assert b'"' not in w[0] and b'"' in w[1]
    def only_strings_in_front(n):
        w = M.window_bytes(D["only strings, then the rest"], n)
        tags, raw = _word_kinds(O.parse(w[0], ndjson=True).tape)
        return set(tags[~raw].tolist()) == set(b'r[]"') and any(b'"n"' in x for x in w[1:])
    assert only_strings_in_front(3) and only_strings_in_front(4)
    # errors
    doc = D["stage 2 first, stage 1 last"]
    for n in (2, 3, 4):
        w = M.window_bytes(doc, n)
        assert O.parse(w[0], ndjson=True).rc == 2 and O.parse(w[-1], ndjson=True).rc == 1
    w = M.window_bytes(D["stage 2 twice"], 2)
    assert [O.parse(x, ndjson=True).rc for x in w] == [2, 2]
    doc = D["string closed in the next shard"]
    w = M.window_bytes(doc, 2)
    assert w[0].count(b'"') % 2 == 1 and w[1].startswith(b"y") and w[1].count(b'"') % 2 == 1
    doc, t = t2("record broken at a newline")
    assert doc[t:t + 1] == b"\n" and M.window_bytes(doc, 2) == [doc[:t], doc[t + 1:]] and doc[:t].endswith(b'{"a":') and doc[t + 1:].startswith(b"1}")
    # the shard alone fails stage 1 (its end is no bracket), the whole message fails stage 2: SJHIP_FLAG_INNER_SHARD
    assert O.parse(doc[:t], ndjson=True).rc == 1 and O.parse(doc, ndjson=True).rc == 2
