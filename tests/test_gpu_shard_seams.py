"""GPU: the sharded ParseND at its seams -- where a cut falls, what a shard loses at its ends, what is rebased -- compared exactly with
the oracle's ParseND of the whole message: tape, Strings.B, message window, return code.

1. The built family of tests/shard_model.py (documents of a few hundred bytes, every seam asserted by tests/test_shard_model.py
   ::test_the_construction_holds) through MultiContext([0] * n), n = 1..8, both copy modes: sjhip_parse_nd_multi has no size
   threshold.  One handle per n is reused across the whole family in a fixed order that alternates full shards, empty shards,
   failing and passing documents; after a failing parse sjhip_fetch_multi refuses; the tape alone and Strings.B alone are fetched too.
2. The path inside the library (ctx.parse / ctx.parse_device, csrc/multi_api.hip parse_nd_big and the DevPeek windows) with
   fixtures.nd_shard_limits(1 MiB, 256 KiB), the smallest the hook allows: documents of 1 228 800 bytes, five shards, built from
   64-byte records plus the pieces below; test_the_construction_holds asserts their placement.
3. find_path / count_where across the seams of the passing in-library document, against the same document parsed whole (a
   MultiContext has no queries: its result is the fetched tape, which is compared whole).

Which emitting variant of stage 2 runs (stage2.hip stage2_launch_emit) is decided by the copy mode, not by the size of a shard:
k_str_emit<false> + k_s2_emit_planes<1, .> with every string copied, k_str_emit<true> + k_s2_emit_planes<2, .> without; every
passing document here runs both with non-zero bases (every shard behind the first).  The third, `wide` (a shard of 4 GiB or
more), cannot be reached with shards of 256 KiB; the per-string form (mode 0) needs a run of more than SURROGATE_WALK_CAP
high-surrogate escapes and is not part of this file."""
import ctypes as C

import numpy as np
import pytest

import fixtures
import oracle_lib as O
import shard_model as M

gpu = pytest.mark.gpu  # (test_the_construction_holds needs none)

# ---- 1. the family through MultiContext ---------------------------------------------------------------------------------------
# full shards / some empty / failing / good, again and again (names of shard_model.DOCS; every document is used once)
ORDER = [
    "strings", "one record", "ff behind records", "target on a newline",
    "numbers like tags", "long record", "stage 2 first, stage 1 last", "target before a newline",
    "nested 12 deep", "two records", "vt behind records", "target after a newline",
    "no strings, then strings", "empty containers", "nel behind records", "target on the CR of CRLF",
    "only strings, then the rest", "scalars in arrays", "nbsp behind records", "target in blank lines",
    "space, tab and CR runs", "ff around the message", "ls behind records", "target in an escaped n",
    "vt around the message", "ff in front of records", "nel around the message", "vt in front of records",
    "nbsp around the message", "nel in front of records", "ls around the message", "nbsp in front of records",
    "strings", "ls in front of records", "scalar roots", "stage 2 twice", "string closed in the next shard",
    "record broken at a newline", "numbers like tags",
]
assert set(ORDER) == set(M.DOCS)

_refs = {}


def ref_of(name, copy):
    if (name, copy) not in _refs:
        _refs[name, copy] = O.parse(M.DOCS[name], ndjson=True, copy_strings=copy)
    return _refs[name, copy]


@gpu
@pytest.mark.parametrize("n", list(M.N_RANGE))
def test_family_through_multicontext(n):
    import sjhip
    from sjhip.api import MultiContext
    L = sjhip.lib()
    m = MultiContext([0] * n)
    try:
        for name in ORDER:
            doc = M.DOCS[name]
            for copy in (True, False):
                ref = ref_of(name, copy)
                try:
                    pj = m.parse_nd(doc, copy_strings=copy)
                    rc = 0
                except sjhip.ParseError as e:
                    rc = e.code
                assert rc == ref.rc, (name, n, copy, rc, ref.rc, M.window_bytes(doc, n))
                if rc != 0:  # nothing to fetch after a failing parse
                    junk = np.zeros(4096, np.uint64)
                    assert L.sjhip_fetch_multi(m._h, junk.ctypes.data, junk.ctypes.data) != 0, (name, n, copy)
                    assert not junk.any()
                    continue
                assert pj.Message == doc[ref.msg_off:ref.msg_off + ref.msg_len], (name, n, copy)
                assert np.array_equal(pj.Tape, ref.tape), (name, n, copy)
                assert np.array_equal(pj.Strings, ref.strings), (name, n, copy)
                # the tape alone, Strings.B alone
                tape = np.zeros(len(ref.tape), np.uint64)
                assert L.sjhip_fetch_multi(m._h, tape.ctypes.data, None) == 0 and np.array_equal(tape, ref.tape), (name, n, copy)
                strings = np.zeros(max(len(ref.strings), 1), np.uint8)
                assert L.sjhip_fetch_multi(m._h, None, strings.ctypes.data) == 0, (name, n, copy)
                assert np.array_equal(strings[:len(ref.strings)], ref.strings), (name, n, copy)
    finally:
        m.close()


# ---- 2. inside the library: five shards of ~240 KiB ----------------------------------------------------------------------------
LIMIT, SHARD = 1 << 20, 256 << 10
WINDOW = 64 << 10                       # multi_api.hip DevPeek
TOTAL = 5 * 245760                      # 1 228 800 bytes: targets at k * 245 760
T = [TOTAL * k // 5 for k in range(6)]
LONG_AT = T[1] - 100 * 1024             # the long record begins 100 KiB in front of target 1 ...
CUT1 = T[1] + 3 * WINDOW                # ... and its newline is the last byte of the third window find_newline reads
CUT2 = T[2] + 64                        # target 2 lies right behind a newline: the cut follows the NEXT one
RUN2_END = CUT2 + 1094 * 64             # 70 016 blanks (spaces and newlines) behind cut 2: the front trim takes a second window
CUT3 = T[3] + 11                        # exactly 65 536 blanks (65 535 spaces, one newline) in front of cut 3
RUN3_AT = CUT3 - WINDOW
CUT4 = T[4] + 64                        # 70 016 blanks in front of cut 4: the back trim takes a second window
RUN4_AT = CUT4 - 1094 * 64
CUTS = [0, CUT1, CUT2, CUT3, CUT4, TOTAL]


def line(i, size=64, tail=b"\n"):
    """a record of `size` bytes with its tail; the id and the string v<id> are unique"""
    head = b'{"id":%07d,"k":"v%07d","pad":"' % (1000000 + i, i)
    return head + b"p" * (size - len(head) - 2 - len(tail)) + b'"}' + tail


def big_document(variant="ok"):
    out, i = [], [0]
    size = [0]

    def put(b):
        out.append(b)
        size[0] += len(b)

    def fill(upto, last_tail=b"\n"):
        """64-byte records up to `upto`; the last one takes up what is left over and ends with last_tail"""
        while upto - size[0] >= 128:
            put(line(i[0]))
            i[0] += 1
        put(line(i[0], upto - size[0], last_tail))
        i[0] += 1

    fill(LONG_AT)
    head = b'{"id":%07d,"k":"v%07d","long":"' % (1000000 + i[0], i[0])
    i[0] += 1
    put(head + b"x" * (CUT1 - LONG_AT - len(head) - 3) + b'"}\n')                       # its newline at CUT1 - 1
    fill(T[2])
    fill(CUT2, b"\x0c\n" if variant == "ff at an end" else b"\n")                         # one record: shard 1 ends here
    put((b" " * 63 + b"\n") * 1094)
    fill(RUN3_AT, b"")                                                                   # no newline: the blanks follow the bracket
    put(b" " * (WINDOW - 1) + b"\n")
    fill(RUN4_AT)
    put((b" " * 63 + b"\n") * 1094)
    if variant == "ff at a start":
        put(b"\x0c" + line(i[0], 63))
        i[0] += 1
    fill(TOTAL, {"ff last": b"\x0c", "nbsp last": b"\xc2\xa0"}.get(variant, b"\n"))
    doc = b"".join(out)
    assert len(doc) == TOTAL
    return doc


VARIANTS = ["ok", "ff at an end", "ff at a start", "ff last", "nbsp last"]
_big = {}


def big(variant):
    if variant not in _big:
        _big[variant] = big_document(variant)
    return _big[variant]


def big_ref(variant, copy):
    key = ("big", variant, copy)
    if key not in _refs:
        _refs[key] = O.parse(big(variant), ndjson=True, copy_strings=copy)
    return _refs[key]


def test_the_construction_holds():
    doc = big("ok")
    assert LIMIT < len(doc) and (len(doc) + SHARD - 1) // SHARD == 5
    assert M.cuts(doc, 5) == CUTS
    # the long record lies across target 1 and its newline ends the third 64 KiB window behind the target
    assert doc[LONG_AT - 1:LONG_AT + 1] == b"\n{" and b"\n" not in doc[LONG_AT:CUT1 - 1] and doc[CUT1 - 1:CUT1] == b"\n"
    assert LONG_AT < T[1] < CUT1 and CUT1 - LONG_AT > 200 * 1024 and (CUT1 - T[1]) % WINDOW == 0 and (CUT1 - T[1]) // WINDOW == 3
    # target 2 right behind a newline
    assert doc[T[2] - 1:T[2] + 1] == b"\n{" and doc.index(b"\n", T[2]) + 1 == CUT2
    # more than 64 KiB of blanks behind cut 2, exactly 64 KiB in front of cut 3, more than 64 KiB in front of cut 4
    assert set(doc[CUT2:RUN2_END]) == set(b" \n") and RUN2_END - CUT2 > WINDOW and doc[RUN2_END:RUN2_END + 1] == b"{"
    assert doc[RUN3_AT - 1:RUN3_AT] == b"}" and doc[RUN3_AT:CUT3] == b" " * (WINDOW - 1) + b"\n" and RUN3_AT + WINDOW - 1 >= T[3]
    assert doc[RUN4_AT - 2:RUN4_AT] == b"}\n" and set(doc[RUN4_AT:CUT4]) == set(b" \n") and CUT4 - RUN4_AT > WINDOW
    assert doc[CUT4 - 1:CUT4 + 1] == b"\n{" and doc[T[4] - 1:T[4]] == b"\n" and doc[T[4]:CUT4 - 1] == b" " * 63
    wins, g_off, g_len = M.windows(doc, 5)
    assert wins == [(0, CUT1 - 1), (CUT1, CUT2 - 1), (RUN2_END, RUN3_AT), (CUT3, RUN4_AT - 1), (CUT4, TOTAL - 1)] and g_off == 0
    for variant in VARIANTS:
        d = big(variant)
        assert M.cuts(d, 5) == CUTS, variant
    w = M.window_bytes(big("ff at an end"), 5)
    assert w[1].endswith(b'"}\x0c') and sum(x.count(b"\x0c") for x in w) == 1
    w = M.window_bytes(big("ff at a start"), 5)
    assert w[4].startswith(b'\x0c{"id"') and sum(x.count(b"\x0c") for x in w) == 1
    assert big("ff last").endswith(b'"}\x0c') and big("nbsp last").endswith(b'"}\xc2\xa0')
    for variant, want in zip(VARIANTS, (0, 2, 2, 0, 0)):
        ref = big_ref(variant, True)
        assert ref.rc == want, variant
        if want == 0:
            assert (ref.msg_off, ref.msg_len) == (0, M.windows(big(variant), 5)[0][4][1]), variant


def _device_copy(data):
    import torch
    d = torch.empty(len(data) + 256, dtype=torch.uint8, device="cuda:0")
    d[:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    torch.cuda.synchronize()
    return d


_ctx = {}


def context():
    import sjhip
    if "c" not in _ctx:
        _ctx["c"] = sjhip.Context(0)
    return _ctx["c"]


@gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_in_library_documents(variant):
    import sjhip
    ctx = context()
    doc = big(variant)
    dev = _device_copy(doc)
    for copy in (True, False):
        ref = big_ref(variant, copy)
        with fixtures.nd_shard_limits(LIMIT, SHARD):
            try:
                pj = ctx.parse(doc, ndjson=True, copy_strings=copy)
                rc = 0
            except sjhip.ParseError as e:
                rc = e.code
        assert rc == ref.rc, (variant, copy, "host", rc)
        if rc == 0:
            assert pj.Message == doc[ref.msg_off:ref.msg_off + ref.msg_len], (variant, copy)
            assert np.array_equal(pj.Tape, ref.tape) and np.array_equal(pj.Strings, ref.strings), (variant, copy, "host")
        # device-resident: cuts and trims through the 64 KiB windows
        with fixtures.nd_shard_limits(LIMIT, SHARD):
            try:
                tl, sl = ctx.parse_device(dev.data_ptr(), len(doc), ndjson=True, copy_strings=copy)
                rc = 0
            except sjhip.ParseError as e:
                rc = e.code
        if variant == "nbsp last":
            # multi_api.hip: "a device-resident message that begins or ends with a multi-byte Unicode blank keeps it (and fails like
            # any other stray byte)": the last shard's end is no bracket, stage 1 -- where the host message parses (above)
            assert ref.rc == 0 and rc == 1, (variant, copy, "device", rc)
            assert O.parse(doc[:-2] + b"x", ndjson=True).rc == 1
            continue
        assert rc == ref.rc, (variant, copy, "device", rc)
        if rc == 0:
            tape, strings = ctx.fetch(tl, sl)
            assert np.array_equal(tape, ref.tape) and np.array_equal(strings, ref.strings), (variant, copy, "device")


# ---- 3. queries across the seams ----------------------------------------------------------------------------------------------
def _last_ids(doc, n):
    """v<id> of the last record of every non-empty shard"""
    out = []
    for w in M.window_bytes(doc, n):
        if w:
            last = w[w.rfind(b"\n") + 1:]
            out.append(last[last.index(b'"k":"') + 5:][:8])
    return out


@gpu
def test_queries_across_the_seams():
    import sjhip
    one = sjhip.Context(0)
    many = context()
    doc = big("ok")
    ids = _last_ids(doc, 5)
    assert len(ids) == 5 and all(i.startswith(b"v") for i in ids)
    for copy in (True, False):
        one.parse(doc, ndjson=True, copy_strings=copy)
        with fixtures.nd_shard_limits(LIMIT, SHARD):
            many.parse(doc, ndjson=True, copy_strings=copy)
        for path in ((b"k",), (b"long",), (b"id",)):
            a, b = many.find_path(*path), one.find_path(*path)
            assert len(a) == doc.count(b'"id"') and np.array_equal(a, b), (path, copy)
        for v in ids:
            assert one.count_where(b"k", v) == 1 and many.count_where(b"k", v) == 1, (v, copy)
    one.close()
