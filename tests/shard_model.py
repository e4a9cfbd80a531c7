"""Host model of the sharded ParseND (csrc/multi_api.hip multi_parse, sjhip/ndshard.py): where the cuts fall, what window every
shard parses, which bases its tape is emitted with and which verdict the shards agree on -- and a family of small, BUILT documents
that put a cut, a trim or a rebased word on every seam of that logic.  TEST INFRASTRUCTURE ONLY.

The rule (csrc/sj_host.h shard_windows):
  cuts     shard k ends right behind the first '\\n' at or after max(previous cut, len * (k + 1) / n); the last ends at len
  window   the cut range, intersected with the bytes.TrimSpace window of the whole message, without space, \\t, \\n, \\r at its ends
           and nothing else; an empty window contributes nothing
  bases    exclusive prefix sums of the shards' (tape_len, strings_len); msg_base = window start - global offset
  verdict  a stage-1 failure of any shard first, then the lowest failing shard's code.  "The last structural is a closing bracket"
           is asked of the end of the MESSAGE: a window that a later non-empty one follows and that ends otherwise is a stage-2
           failure unless stage 1 finds another fault (SJHIP_FLAG_INNER_SHARD)
windows() restates the first two in Python (the global TrimSpace is the oracle's), merged() runs all four with the host replay
of the kernels (csrc/host_selftest.cpp sj_selftest_parse_shard) standing in for the device."""
import ctypes as C
import struct

import numpy as np

import oracle_lib as O

JSON_WS = b" \t\n\r"
FLAG_INNER = 8
_LIB = None


def selftest(path=None):
    """the host replay library (built from the tree, or `path`: another build of it)"""
    global _LIB
    if path is None and _LIB is not None:
        return _LIB
    if path is None:
        import __graft_entry__ as G
        path = G.build_selftest()
    lib = C.CDLL(path)
    szp, u64pp, u8pp = C.POINTER(C.c_size_t), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint8))
    lib.sj_selftest_parse_shard.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, u64pp,
                                            szp, u8pp, szp, szp, szp]
    lib.sj_selftest_parse_shard.restype = C.c_int
    lib.sj_selftest_trim.argtypes = [C.c_char_p, C.c_size_t, szp, szp]
    lib.sj_selftest_free.argtypes = [C.c_void_p]
    if hasattr(lib, "sj_selftest_shard_windows"):
        lib.sj_selftest_shard_windows.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, szp, szp, C.c_char_p, szp, szp]
        lib.sj_selftest_shard_windows.restype = None
    _LIB = lib
    return lib


# ---- the rule -------------------------------------------------------------------------------------------------------------
def trim_space(doc):
    """bytes.TrimSpace(doc) -> (off, len), by the oracle"""
    off, ln = C.c_size_t(0), C.c_size_t(0)
    O.lib().sjo_trim_space(doc, len(doc), C.byref(off), C.byref(ln))
    return off.value, ln.value


def targets(doc, n):
    """len * k / n for k = 1 .. n - 1: where the search for the newline of cut k starts, unless the previous cut lies behind it"""
    return [len(doc) * k // n for k in range(1, n)]


def cuts(doc, n):
    out = [0]
    for t in targets(doc, n):
        j = doc.find(b"\n", max(out[-1], t))
        out.append(len(doc) if j < 0 else j + 1)
    out.append(len(doc))
    return out


def windows(doc, n):
    """-> ([(start, end) of every shard's window], g_off, g_len)"""
    g_off, g_len = trim_space(doc)
    c = cuts(doc, n)
    out = []
    for a, b in zip(c, c[1:]):
        a, b = max(a, g_off), min(b, g_off + g_len)
        while a < b and doc[a] in JSON_WS:
            a += 1
        while b > a and doc[b - 1] in JSON_WS:
            b -= 1
        out.append((a, max(a, b)))
    return out, g_off, g_len


def inner(wins):
    """per shard: a later window holds something"""
    return [any(b > a for a, b in wins[k + 1:]) for k in range(len(wins))]


def cpp_windows(doc, n, lib=None):
    """the same through the exported C++ rule -> (windows, inner, g_off, g_len)"""
    lib = lib or selftest()
    if not hasattr(lib, "sj_selftest_shard_windows"):
        # a library from before the rule (profiles/r39_shard_seams_cpu.txt): every cut range through its own TrimSpace
        def trim(b, base=0):
            off, ln = C.c_size_t(0), C.c_size_t(0)
            lib.sj_selftest_trim(b, len(b), C.byref(off), C.byref(ln))
            return base + off.value, base + off.value + ln.value
        c = cuts(doc, n)
        wins = [trim(doc[a:b], a) for a, b in zip(c, c[1:])]
        g = trim(doc)
        return wins, inner(wins), g[0], g[1] - g[0]
    starts, lens = (C.c_size_t * n)(), (C.c_size_t * n)()
    inn = C.create_string_buffer(n)
    go, gl = C.c_size_t(0), C.c_size_t(0)
    lib.sj_selftest_shard_windows(doc, len(doc), n, starts, lens, inn, C.byref(go), C.byref(gl))
    return [(starts[k], starts[k] + lens[k]) for k in range(n)], [b != 0 for b in inn.raw[:n]], go.value, gl.value


# ---- the merge --------------------------------------------------------------------------------------------------------------
def replay(window, flags, tb=0, sb=0, mb=0, lib=None):
    """one window through the host replay -> (rc, tape, strings)"""
    lib = lib or selftest()
    tape, strs = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)()
    tl, sl, mo, ml = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    rc = lib.sj_selftest_parse_shard(window, len(window), flags, tb, sb, mb, C.byref(tape), C.byref(tl), C.byref(strs), C.byref(sl),
                                     C.byref(mo), C.byref(ml))
    if rc != 0:
        return rc, np.zeros(0, np.uint64), np.zeros(0, np.uint8)
    t = np.ctypeslib.as_array(tape, shape=(max(tl.value, 1),))[: tl.value].copy()
    s = np.ctypeslib.as_array(strs, shape=(max(sl.value, 1),))[: sl.value].copy()
    lib.sj_selftest_free(tape)
    lib.sj_selftest_free(strs)
    return 0, t, s


def bases(sizes):
    out, t, s = [], 0, 0
    for tl, sl in sizes:
        out.append((t, s))
        t += tl
        s += sl
    return out


def verdict(codes):
    """what the shards agree on: stage 1 of any shard first, then the lowest failing shard's code"""
    if 1 in codes:
        return 1
    return next((c for c in codes if c), 0)


def msg_base(start, g_off):
    return start - g_off


def merged(doc, n, copy, lib=None):
    """-> (rc, tape, strings, g_off, g_len): the document parsed in n shards by the rule, on the host"""
    flags = 1 | (2 if copy else 0)
    wins, g_off, g_len = windows(doc, n)
    if g_len == 0:
        return 1, np.zeros(0, np.uint64), np.zeros(0, np.uint8), g_off, g_len
    inn = inner(wins)
    first = [replay(doc[a:b], flags | (FLAG_INNER if i else 0), lib=lib) if b > a else (0, (), ()) for (a, b), i in zip(wins, inn)]
    rc = verdict([r for r, _, _ in first])
    if rc:
        return rc, np.zeros(0, np.uint64), np.zeros(0, np.uint8), g_off, g_len
    tapes, strs, codes = [], [], []
    for ((a, b), (tb, sb)) in zip(wins, bases([(len(t), len(s)) for _, t, s in first])):
        if b > a:
            r, t, s = replay(doc[a:b], flags, tb, sb, msg_base(a, g_off), lib=lib)
            codes.append(r)
            tapes.append(t)
            strs.append(s)
    rc = verdict(codes)
    if rc:
        return rc, np.zeros(0, np.uint64), np.zeros(0, np.uint8), g_off, g_len
    return 0, np.concatenate(tapes), np.concatenate(strs), g_off, g_len


# ---- the documents ----------------------------------------------------------------------------------------------------------
def rec(i, size):
    """a record of exactly `size` bytes (>= 12)"""
    head = b'{"r%d":"' % (i % 10)
    assert size >= len(head) + 2
    return head + b"p" * (size - len(head) - 2) + b'"}'


BLANKS = {"vt": b"\x0b", "ff": b"\x0c", "nel": b"\xc2\x85", "nbsp": b"\xc2\xa0", "ls": b"\xe2\x80\xa8"}
DEEP12 = b"[" * 12 + b'{"k":[1,"\\u00e9",{"z":null}]}' + b"]" * 12
F22 = struct.unpack("<d", struct.pack("<Q", 0x2200000000000003))[0]   # doubles whose bits begin with the tags '"' and '{'
F7B = struct.unpack("<d", struct.pack("<Q", 0x7B0F000000000000))[0]


def _documents():
    d = {}
    r = rec
    # where the target falls (n = 2 unless said otherwise: the target is len // 2)
    d["target on a newline"] = r(0, 40) + b"\n" + r(1, 40)                                  # 81 bytes, [40] = \n
    d["target before a newline"] = r(0, 41) + b"\n" + r(1, 39)                              # 81 bytes, [41] = \n
    d["target after a newline"] = r(0, 39) + b"\n" + r(1, 20) + b"\n" + r(2, 20)            # 81 bytes, [39] = \n
    d["target on the CR of CRLF"] = r(0, 40) + b"\r\n" + r(1, 39)                           # 81 bytes, [40] = \r
    d["target in blank lines"] = r(0, 38) + b"\n\n\n\n\n" + r(1, 38)                        # 81 bytes, [38..42] = \n
    d["target in an escaped n"] = b'{"s":"' + b"a" * 34 + b'\\n' + b"b" * 24 + b'"}\n' + r(1, 12)
    # n = 8: targets 1 .. 7 lie inside record 1, so the searches behind it start at the previous cut: blank lines give empty shards
    d["long record"] = r(0, 12) + b"\n" + r(1, 200) + b"\n\n\n" + r(2, 12) + b"\n" + r(3, 12)
    d["one record"] = b"  " + r(0, 60) + b" "
    d["two records"] = r(0, 20) + b"\n" + r(1, 20)                                          # n = 3 .. 8: fewer records than shards
    # what lies at a shard's edge
    for name, w in BLANKS.items():
        d["%s behind records" % name] = b"".join(b'{"a":%d}' % k + w + b"\n" for k in range(4))[:-1 - len(w)]
        d["%s in front of records" % name] = b'{"a":0}' + b"".join(b"\n" + w + b'{"a":%d}' % k for k in range(1, 4))
        d["%s around the message" % name] = w + b'{"s":"x\\ty","t":"plain"}\n{"u":"v"}\n' + r(3, 30) + w
    d["space, tab and CR runs"] = (b" \t\r\n" + r(0, 20) + b" \t \r\n\r\n \t" + r(1, 20) + b"\t\t\n   \n\r\r\n" + r(2, 20) + b" \r\n\t")
    # what is rebased
    d["scalar roots"] = b'{"a":1}\n1\n"s"\ntrue\n{"b":2}'                                   # (the reference's ParseND rejects them)
    d["scalars in arrays"] = b'{"e":[]}\n[1]\n["s"]\n[true]\n[null]\n[1.5]\n[-7]'
    d["empty containers"] = b'{}\n[]\n{}\n[]\n[[]]\n[{}]\n[]\n{}'
    d["nested 12 deep"] = r(0, 30) + b"\n" + DEEP12 + b"\n" + DEEP12 + b"\n" + r(1, 30)
    d["strings"] = b"".join(b'{"k%d":"plain%d","e":"q\\"%d\\u00e9\\n","u":"\\ud83d\\ude00"}\n' % (k, k, k) for k in range(6))
    d["numbers like tags"] = b"\n".join(b"[%d,%d,%d,%s,%s]" % (v - 1, v, v + 1, repr(F22).encode(), repr(F7B).encode())
                                        for v in (8863084066665136128, 6557241057451442176, 8214565720323784704, 2449958197289549824))
    d["no strings, then strings"] = b"[1,2,3]\n[4,[5,6]]\n[7.5,null,true]\n" * 2 + b'{"s":"x","t":"a\\tb"}\n' * 3
    d["only strings, then the rest"] = b'["a","b\\n","c"]\n["dd","e"]\n' * 2 + b'{"n":[1,2,{"m":3}]}\n' * 3
    # errors
    good = b'{"a":[1,2,{"b":"c"}]}\n'
    d["stage 2 first, stage 1 last"] = b'{"a":tru}\n' + good * 4 + b'{"z":"unterminated'
    d["stage 2 twice"] = b'{"a":[1,2}\n' + good * 3 + b'{"b":}\n' + good
    d["string closed in the next shard"] = good + b'{"s":"' + b"x" * 20 + b"\n" + b"y" * 20 + b'"}\n' + good
    d["record broken at a newline"] = r(0, 34) + b'\n{"a":\n1}\n' + r(1, 36)                # 80 bytes, [40] = the \n inside
    return d


DOCS = _documents()
N_RANGE = range(1, 9)


def window_bytes(doc, n):
    return [doc[a:b] for a, b in windows(doc, n)[0]]
