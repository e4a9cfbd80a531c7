"""Where the string pass cuts a message, documents that put a string hazard exactly on those cuts, and an independent
model of what the pass must produce.  No GPU import, no oracle import.

The string path (csrc/sj_strings.h, the string half of csrc/stage2.hip: str_masks_body / k_measure, k_scans,
str_emit_body / k_str_emit) works on 64-byte chunks (one per lane), 4 KiB units (one per wave), blocks of four waves,
and -- WithCopyStrings(false) -- walks over the unit flags in steps of 64 units.  Chunks count from the 64-byte aligned
base of the message: byte i of a message at lead `lead` has the aligned offset lead + i.  Across every cut something
is handed over: a \\uXXXX whose 'u' lies in the last four bytes of a chunk reaches into the next one (a "foreign item"
of the next unit, GEN_FOREIGN), the emitted prefix of a unit decides where a chunk's bytes land in an 8-byte LDS slot,
and whether a string is copied without copy_strings is a carry chain over the chunks of a unit seeded by two walks over
the units in front and behind.

Every placement here is exact (blanks are the filler, as in s1_geometry.byte_doc) and a placement that does not fit
raises: no document is ever left out.  tests/test_str_geometry.py checks on the CPU that the documents cover what
they claim, that the oracle gives them the verdict they claim, that the model below agrees with the oracle, and runs
them through the host replay; tests/test_gpu_string_seams.py runs them on the device.

The model (string_tokens / expected_strings / emit_mask) is a tokenizer of a dozen lines plus json.loads per string
token.  It shares no code with the kernels or with oracle/ and is only defined for the documents marked `plain`
(valid, none of the reference's quirks)."""
import collections
import json
import re

import numpy as np

CHUNK = 64
UNIT = 4096
BLOCK_UNITS = 4     # k_measure / k_str_emit: four waves per block, unit = 4 * block + wave (then + the grid's waves)
SEL_STEP_UNITS = 64  # sel_unit_in / sel_unit_out: 64 unit flags per step

Doc = collections.namedtuple("Doc", "name data nd plain info")


# ---- the model ---------------------------------------------------------------------------------------------------------
_STRING = re.compile(rb'"[^"\\]*(?:\\.[^"\\]*)*"', re.S)
_ESCAPE = re.compile(rb"\\(?:u([0-9a-fA-F]{4})|.)", re.S)


def string_tokens(doc):
    """(index of the opening quote, index of the closing quote) of every string of `doc`, in document order"""
    return [(m.start(), m.end() - 1) for m in _STRING.finditer(bytes(doc))]


def expected_strings(doc, copy):
    """Strings.B of a plain document: the UTF-8 of every string in document order (copy), or only of the strings that
    contain a backslash (WithCopyStrings(false))"""
    doc = bytes(doc)
    out = bytearray()
    for o, c in string_tokens(doc):
        if copy or b"\\" in doc[o + 1:c]:
            out += json.loads(doc[o:c + 1].decode("ascii")).encode("utf-8")
    return bytes(out)


def emit_mask(doc, copy=True):
    """per byte of a plain document: does Strings.B receive a byte from this position?  Plain content and the character
    behind a simple escape emit at their own position; a \\uXXXX that encodes to n bytes emits at 'u' and the n - 1
    digits behind it; a surrogate pair emits four bytes at the high half and none at the low half."""
    doc = bytes(doc)
    em = np.zeros(len(doc), dtype=bool)
    for o, c in string_tokens(doc):
        if not (copy or b"\\" in doc[o + 1:c]):
            continue
        em[o + 1:c] = True
        low_half = -1
        for m in _ESCAPE.finditer(doc, o + 1, c):
            i = m.start()
            em[i] = False
            if m.group(1) is None:
                continue
            cp = int(m.group(1), 16)
            n = 0 if i == low_half else 4 if 0xD800 <= cp < 0xDC00 else 1 if cp < 0x80 else 2 if cp < 0x800 else 3
            if n == 4:
                low_half = i + 6
            em[i + 1 + n:i + 6] = False
    return em


def unit_emit_counts(doc, lead=0, copy=True):
    em = emit_mask(doc, copy)
    a = np.zeros((lead + len(em) + UNIT - 1) // UNIT * UNIT, dtype=np.int64)
    a[lead:lead + len(em)] = em
    return a.reshape(-1, UNIT).sum(axis=1)


def compaction_cases(doc, lead=0):
    """what the compaction of k_str_emit sees (copy mode): per aligned 8-byte group of a chunk that emits anything, the
    emitted bytes of the unit in front of the group mod 8 and the two 4-bit emit patterns of the byte pair
    -> set of (pattern, offset mod 8, nibble position)"""
    em = emit_mask(doc)
    a = np.zeros((lead + len(em) + UNIT - 1) // UNIT * UNIT, dtype=np.int64)
    a[lead:lead + len(em)] = em
    out = set()
    for u in range(0, a.size, UNIT):
        unit = a[u:u + UNIT]
        before = np.concatenate(([0], np.cumsum(unit)))
        for c in range(0, UNIT, CHUNK):
            if not unit[c:c + CHUNK].any():
                continue
            for g in range(c, c + CHUNK, 8):
                for pos in (0, 1):
                    nib = unit[g + 4 * pos:g + 4 * pos + 4]
                    out.add((int(nib[0] + 2 * nib[1] + 4 * nib[2] + 8 * nib[3]), int(before[g]) & 7, pos))
    return out


# ---- placement ---------------------------------------------------------------------------------------------------------
def place_doc(length, items, nd=False, fill=0x20):
    """A document of exactly `length` bytes: '[' first, ']' last, every (offset, text) of `items` at its offset as one
    array element (plain: ``[ e0, e1 ]``; nd: one record ``[ e ]`` per element), blanks elsewhere.  An item that
    overlaps its neighbour or the ends of the message is an error of the caller."""
    sep = b"]\n[" if nd else b","
    a = bytearray([fill]) * length
    a[0], a[length - 1] = 0x5B, 0x5D
    items = sorted(items)
    free = 1
    for i, (at, text) in enumerate(items):
        last = i + 1 == len(items)
        end = at + len(text)
        if at < free or end + (0 if last else len(sep)) > length - 1:
            raise ValueError(("does not fit", at, text, free, length))
        a[at:end] = text
        if not last:
            a[end:end + len(sep)] = sep
        free = end + len(sep)
    return bytes(a)


Hazard = collections.namedtuple("Hazard", "name pre haz post owns_open owns_close")


def _hz(name, haz, pre=b"p", post=b"q", owns_open=False, owns_close=False):
    return Hazard(name, b"" if owns_open else pre, haz, b"" if owns_close else post, owns_open, owns_close)


def element(h, form="value", post=None):
    """-> (text of one array element, index of the hazard's first byte in it).  form "key": the string is an object key"""
    post = h.post if post is None else post
    s = (b"" if h.owns_open else b'"' + h.pre) + h.haz + (b"" if h.owns_close else post + b'"')
    lo = 0 if h.owns_open else 1 + len(h.pre)
    if form == "key":
        return b"{" + s + b":1}", lo + 1
    return s, lo


SIMPLE_LETTERS = b'"\\/bfnrt'
VALID_HAZARDS = [_hz("simple_" + chr(c), b"\\" + bytes([c])) for c in SIMPLE_LETTERS] + [
    _hz("u_1byte", b"\\u0041"), _hz("u_2byte", b"\\u00e9"), _hz("u_3byte", b"\\u20ac"),
    _hz("pair", b"\\ud83d\\ude00"),
    _hz("bs_then_close", b'x\\\\"', pre=b"", owns_close=True),      # x \\ and the closing quote
    _hz("bs_escaped_quote", b'x\\\\\\"y'),                           # x \\ \" y
    _hz("adjacent", b"\\n\\u00e9\\t\\u20ac"),
    _hz("empty", b'""', owns_open=True, owns_close=True),
    _hz("open_quote", b'"', post=b"abc", owns_open=True),             # split 1: the opening quote is the last byte in front
    _hz("close_quote", b'"', pre=b"abc", owns_close=True),            # split 0: the closing quote is the first byte behind
]
ERROR_HAZARDS = [_hz("bad_letter", b"\\a")] + [
    _hz("nonhex_%d" % i, b"\\u" + b"0041"[:i] + b"G" + b"0041"[i + 1:]) for i in range(4)] + [
    _hz("cut_%d" % n, b"\\u" + b"123"[:n] + b'"', owns_close=True) for n in (1, 2, 3)] + [
    _hz("high_then_plain", b"\\ud83dx"),
    _hz("high_then_close", b'\\ud83d"', owns_close=True),
    _hz("high_then_simple", b"\\ud83d\\n"),
]
FORMS = ("value", "key")


def splits(h):
    """the seam falls in front of byte s of the hazard, s = 0 .. n - 1, or directly behind it (s = n)"""
    return range(len(h.haz) + 1)


def place_on_seam(h, form, s, seam, lead=0, post=None):
    """(message offset, element text) so that byte s of the hazard is the first byte behind the cut at aligned `seam`"""
    text, lo = element(h, form, post)
    return seam - lead - lo - s, text


COMBOS = [(h, s, f) for f in FORMS for h in VALID_HAZARDS for s in splits(h)]
END_CASES = [(h, f, e) for f in FORMS for h in VALID_HAZARDS for e in range(4)]

# ---- rotation documents ------------------------------------------------------------------------------------------------
SEAM_CLASSES = ("chunk", "unit", "block", "first", "last", "end")
ROT_UNITS = 10
ROT_LENGTH = (ROT_UNITS - 1) * UNIT + 1500  # the last unit is partial
_ROT_CHUNK_SEAMS = ((0, 31), (1, 63), (2, 1), (3, 32), (5, 17), (6, 62))  # (unit, chunk): lanes low, high and in between


def rotation_seams():
    """(class, aligned offset of the first byte behind the cut) of every cut a rotation document carries a hazard on:
    first = the first chunk seam of the message, chunk = chunk seams inside a unit, unit = unit seams inside a block,
    block = unit seams between two blocks, last = the seam in front of the partial last unit"""
    out = [("first", CHUNK)]
    out += [("chunk", u * UNIT + c * CHUNK) for u, c in _ROT_CHUNK_SEAMS]
    for u in range(1, ROT_UNITS):
        out.append(("last" if u == ROT_UNITS - 1 else "block" if u % BLOCK_UNITS == 0 else "unit", u * UNIT))
    return out


def rotation_layout(k):
    """what document k of the rotation carries: [(class, seam, hazard, split, form)] and its message-end case
    (hazard, form, e).  Seam i carries combination (k + 13 i) mod len(COMBOS): over k = 0 .. len(COMBOS) - 1 every seam
    carries every combination once."""
    lay = [(cls, seam) + COMBOS[(k + 13 * i) % len(COMBOS)] for i, (cls, seam) in enumerate(rotation_seams())]
    return lay, END_CASES[k % len(END_CASES)]


def end_element(h, form, e):
    """the hazard ends e bytes in front of the closing quote + bracket of the message (a hazard that owns its closing
    quote: e blanks between that quote and the bracket) -> (text, blanks behind it)"""
    if h.owns_close:
        return element(h, form)[0], e
    return element(h, form, b"q" * e)[0], 0


def rotation_doc(k, nd):
    lay, (eh, ef, ee) = rotation_layout(k)
    items = [place_on_seam(h, f, s, seam) for _, seam, h, s, f in lay]
    text, blanks = end_element(eh, ef, ee)
    items.append((ROT_LENGTH - 1 - blanks - len(text), text))
    return Doc("rotation %d%s" % (k, " nd" if nd else ""), place_doc(ROT_LENGTH, items, nd), nd, True, (lay, (eh, ef, ee)))


def rotation_docs(nd):
    return (rotation_doc(k, nd) for k in range(len(COMBOS)))


# ---- the chunk-seam family for a device pointer that is not 64-byte aligned -----------------------------------------------
def lead_layout(lead):
    """every combination on a chunk seam (never a unit seam) of one message at `lead`: [(seam, hazard, split, form)]"""
    out = []
    c = 2
    for h, s, f in COMBOS:
        if c % 64 == 0:
            c += 1
        out.append((c * CHUNK, h, s, f))
        c += 1
    return out


def lead_doc(lead, nd):
    lay = lead_layout(lead)
    length = lay[-1][0] + 200 - lead
    items = [place_on_seam(h, f, s, seam, lead) for seam, h, s, f in lay]
    return Doc("chunk seams at lead %d%s" % (lead, " nd" if nd else ""), place_doc(length, items, nd), nd, True, (lead, lay))


# ---- error documents -----------------------------------------------------------------------------------------------------
ERROR_CLASSES = ("chunk", "unit", "block")
_OK_HEAD = b'"ok\\n\\u00e9"'


def error_seam(cls, s):
    """(aligned seam, document length): chunk -- a chunk seam of the first of two units (another lane for every split);
    unit -- the seam between two units; block -- the seam between units 3 and 4, the smallest message that has one"""
    if cls == "chunk":
        return CHUNK * (2 + (11 * s) % 60), UNIT + 1500
    if cls == "unit":
        return UNIT, UNIT + 1500
    return BLOCK_UNITS * UNIT, BLOCK_UNITS * UNIT + 1500


def one_hazard_doc(h, form, s, cls):
    """one hazard on one seam, a valid escaped string at both ends of the message: the hazard decides the verdict"""
    seam, length = error_seam(cls, s)
    items = [(2, _OK_HEAD), place_on_seam(h, form, s, seam), (length - 2 - len(_OK_HEAD), _OK_HEAD)]
    return place_doc(length, items)


def error_docs():
    for h in ERROR_HAZARDS:
        for s in splits(h):
            for cls in ERROR_CLASSES:
                form = FORMS[(s + len(cls)) % 2]
                yield Doc("error %s split %d %s %s" % (h.name, s, cls, form), one_hazard_doc(h, form, s, cls), False, False,
                          (h.name, s, cls))


def quirk_hazard(body):
    """a body of tests/golden/strings.json as a hazard: from its first backslash to its closing quote"""
    at = body.index(b"\\")
    return _hz("golden", body[at:] + b'"', pre=body[:at], owns_close=True)


def quirk_docs(bodies):
    """the bodies of the reference's string table that hold an escape, on the seams; the verdict is the oracle's on the
    bare document bare_doc(body)"""
    for i, body in enumerate(bodies):
        if b"\\" not in body:
            continue
        h = quirk_hazard(body)
        for s in splits(h):
            for cls in ERROR_CLASSES:
                yield Doc("golden %d split %d %s" % (i, s, cls), one_hazard_doc(h, "value", s, cls), False, False, (i, s, cls))


def bare_doc(body):
    return b'["' + body + b'"]'


# ---- compaction documents (copy mode) -------------------------------------------------------------------------------------
# pattern (bit i = byte i of the nibble emits) -> (array elements, index of the nibble's first byte).  A one is a byte inside
# a string that is no quote and no backslash; a zero is a quote, a backslash or a byte outside.  1001 cannot be written with
# simple escapes (a backslash is followed by an emitted byte, a closing quote by at least two more zeros): it is the tail of
# a three-byte \u escape.
NIBBLES = {
    0b0000: (b'"a"    ,"a"', 3), 0b1111: (b'"abcd"', 1), 0b0001: (b'"a"   ', 1), 0b0010: (b'"a" ', 0),
    0b0100: (b' "a"', 0), 0b1000: (b'  "a"', 0), 0b0011: (b'"ab"  ', 1), 0b0110: (b'"ab" ', 0),
    0b1100: (b' "ab"', 0), 0b0111: (b'"abc" ', 1), 0b1110: (b'"abc"', 0), 0b0101: (b'"a\\n"', 1),
    0b1010: (b'"\\n\\n"', 1), 0b1101: (b'"a\\nb"', 1), 0b1011: (b'"ab\\n"', 1), 0b1001: (b'"\\u20acx"', 4),
}


def _pad_string(n, i):
    """a string that emits n mod 8 bytes: lengths 0 .. 9, with and without a simple escape, every escaped letter in turn"""
    n += 8 if n < 2 and i % 3 == 0 else 0
    if n and i % 2:
        return b'"' + b"x" * (n - 1) + b"\\" + SIMPLE_LETTERS[i % 8:i % 8 + 1] + b'"'
    return b'"' + b"x" * n + b'"'


def compaction_doc(pattern, start):
    """for one emit pattern: the sixteen cases (offset mod 8) x (nibble position), from message offset `start` on"""
    seg, k = NIBBLES[pattern]
    seg_em = emit_mask(seg)
    buf = bytearray(b"[" + b" " * (start - 1))
    i = 0
    for o in range(8):
        for pos in (0, 1):
            while True:
                cur = len(buf)
                s0 = (cur + 14 + k + 7) // 8 * 8 + 4 * pos - k  # room for the longest pad string and its comma
                if cur // UNIT == (s0 + len(seg)) // UNIT:
                    break
                buf += b" " * ((cur // UNIT + 1) * UNIT - cur)  # the whole case inside one unit
            g = s0 + k - 4 * pos  # the aligned group
            ustart = g // UNIT * UNIT
            have = int(emit_mask(bytes(buf))[ustart:].sum()) + int(seg_em[:max(0, g - s0)].sum())
            pad = _pad_string((o - have) % 8, i)
            i += 1
            buf += pad + b","
            buf += b" " * (s0 - len(buf)) + seg + b","
    buf[-1:] = b"]"
    return Doc("compaction %s from %d" % (format(pattern, "04b"), start), bytes(buf), False, True, pattern)


def compaction_docs():
    for pattern in sorted(NIBBLES):
        for start in (1, UNIT + 50 * CHUNK + 3):  # low lanes of the first unit; high lanes of the second, on into the third
            yield compaction_doc(pattern, start)


DENSEST_STRINGS = UNIT // 3  # "", "", ... : three bytes per string


def unit_count_doc():
    """units that emit exactly 0, 1, 4095 and 4096 bytes, and a unit of the densest legal string count"""
    items = [(2, b'"head\\t"'),
             (1 * UNIT + 7, b'""'),                                   # unit 1: nothing
             (2 * UNIT + 2000, b'"a"'),                               # unit 2: one byte
             (3 * UNIT, b'"' + b"y" * (2 * UNIT + 99) + b"\\n" + b"z" * (UNIT - 101) + b'"'),
             # unit 3: the opening quote, then 4095 bytes; unit 4: 4096; unit 5: 4095 (one starter); unit 6: one byte and the quote
             (7 * UNIT, b",".join([b'""'] * (UNIT // 3 * 2)))]        # units 7 and 8: "","", ...
    data = place_doc(9 * UNIT + 300, items)
    return Doc("unit counts", data, False, True, None)


# ---- patch-path documents ----------------------------------------------------------------------------------------------------
def _unit_string(edits, n_units=1):
    """one string from 10 bytes in front of unit 1 to 10 bytes behind unit n_units: {aligned offset: bytes}"""
    o, c = UNIT - 10, (1 + n_units) * UNIT + 10
    body = bytearray(b"x" * (c - o - 1))
    for at, b in edits.items():
        assert all(ch == 0x78 for ch in body[at - o - 1:at - o - 1 + len(b)]), at
        body[at - o - 1:at - o - 1 + len(b)] = b
    return place_doc(c + 100, [(5, b'"h"'), (o, b'"' + bytes(body) + b'"')])


def patch_docs():
    """(1) a unit whose escapes are all simple, one per escaped letter; (2) the same with one chunk of \\u escapes, so that
    a general unit also holds patched chunks that are not general; both with an escape as the first and as the last
    emitted byte of the unit"""
    spread = {UNIT + CHUNK * (3 + 7 * i) + 5 * i: b"\\" + SIMPLE_LETTERS[i:i + 1] for i in range(8)}
    uchunk = {UNIT + CHUNK * 20 + 8: b"\\u00e9\\u20ac\\u0041\\ud83d\\ude00"}
    for mix, base in (("simple", spread), ("mixed", {**spread, **uchunk})):
        yield Doc("patch %s" % mix, _unit_string(base), False, True, mix)
        for i in range(8):
            esc = b"\\" + SIMPLE_LETTERS[i:i + 1]
            for where, at in (("first", UNIT), ("first, starter in front", UNIT - 1), ("last", 2 * UNIT - 2)):
                yield Doc("patch %s %r %s" % (mix, esc, where), _unit_string({**base, at: esc}), False, True, mix)
    for u, n in ((b"\\u0041", 1), (b"\\u00e9", 2), (b"\\u20ac", 3), (b"\\ud83d\\ude00", 4)):
        for where, at in (("first", UNIT), ("first, foreign", UNIT - 1), ("last", 2 * UNIT - 1 - n)):
            # (last: the n emitted positions u, X.. end on the last byte of the unit, the rest of the escape is foreign)
            yield Doc("patch \\u %r %s" % (u, where), _unit_string({**spread, at: u}), False, True, "mixed")


# ---- selective-copy documents --------------------------------------------------------------------------------------------------
def sel_chunk_docs():
    """(a) one chunk holding four strings, all 16 patterns of which of them hold a starter; `inside`: the four strings lie in
    the chunk; `across`: the first began in the chunk in front and the last ends in the chunk behind, and their starter
    lies in that neighbouring chunk only.  The chunk is a middle lane, the first and the last chunk of a unit."""
    for c in (5, 64, 127):
        base = c * CHUNK
        for pat in range(16):
            e = [b"\\n" if (pat >> j) & 1 else b"mn" for j in range(4)]
            inside = [(base + 2, b'"a' + e[0] + b'b"'), (base + 12, b'"' + e[1] + b'"'), (base + 24, b'"cd' + e[2] + b'"'),
                      (base + 40, b'"' + e[3] + b'ef"')]
            across = [(base - 30, b'"' + e[0] + b"g" * 36 + b'"'), inside[1], inside[2],
                      (base + 50, b'"' + b"h" * 30 + e[3] + b'"')]
            for name, items in (("inside", inside), ("across", across)):
                yield Doc("four strings %s chunk %d pattern %s" % (name, c, format(pat, "04b")),
                          place_doc(base + 300, [(2, b'"lead"')] + items), False, True, (name, c, pat))


SEL_UNITS = (1, 2, 3, 63, 64, 65, 66, 128, 129)
SEL_PLACES = ("first", "last", "middle", "from_open_64", "from_close_64", "absent")
_OPEN_AT = UNIT + 2000  # the long string's opening quote; its closing quote lies n units further


def sel_place_applies(n, place):
    """a unit 64 units from a quote only exists inside a string that spans that many"""
    return n >= SEL_STEP_UNITS or place not in ("from_open_64", "from_close_64")


def sel_starter_at(n, place):
    """aligned offset of the long string's only starter (a \\n), or None"""
    close = _OPEN_AT + n * UNIT
    return {"first": _OPEN_AT + 1, "last": close - 2, "middle": _OPEN_AT + n * UNIT // 2,
            "from_open_64": (1 + SEL_STEP_UNITS) * UNIT + 1000, "from_close_64": (1 + n - SEL_STEP_UNITS) * UNIT + 3000,
            "absent": None}[place]


def sel_long_doc(n, place):
    """(b) a string that spans n units -- its quotes lie n units apart -- whose only starter is at `place`; short plain and
    escaped strings in front of it and behind it, in the units of its quotes.
    info: (n, place, units from the opening quote to the starter, units from the starter to the closing quote)"""
    assert sel_place_applies(n, place)
    close = _OPEN_AT + n * UNIT
    body = bytearray(b"w" * (close - _OPEN_AT - 1))
    at = sel_starter_at(n, place)
    dist = None
    if at is not None:
        body[at - _OPEN_AT - 1:at - _OPEN_AT + 1] = b"\\n"
        dist = (at // UNIT - _OPEN_AT // UNIT, close // UNIT - at // UNIT)
    items = [(UNIT + 100, b'"s"'), (UNIT + 200, b'"e\\n"'), (UNIT + 1900, b'"t"'), (_OPEN_AT, b'"' + bytes(body) + b'"'),
             (close + 10, b'"u"'), (close + 100, b'"f\\t\\u00e9"'), (close + 300, b'"v"')]
    return Doc("long string %d units, starter %s" % (n, place), place_doc(close + 500, items), False, True, (n, place, dist))


def sel_long_docs(max_units=None):
    for n in SEL_UNITS:
        if max_units is not None and n > max_units:
            continue
        for place in SEL_PLACES:
            if sel_place_applies(n, place):
                yield sel_long_doc(n, place)


def sel_message_docs():
    """(c) a message without any starter (stage 1's flag, the no_escapes shortcut), and the same message with exactly one
    starter in its first string, in its last string, and in a key"""
    for where in ("none", "first", "last", "key"):
        parts = ['"first%s"' % ("\\n" if where == "first" else "")]
        for i in range(400):
            k = "key%d%s" % (i, "\\t" if where == "key" and i == 217 else "")
            parts.append('{"%s":"value %d %s"}' % (k, i, "z" * (i % 37)))
        parts.append('"last%s"' % ("\\r" if where == "last" else ""))
        yield Doc("message with starter: %s" % where, ("[" + ", ".join(parts) + "]").encode(), False, True, where)


def sel_quote_docs():
    """(d) a closing quote as byte 0 of a unit, an opening quote as byte 4095 of a unit, with and without a starter in the
    string on the far side of the seam"""
    for starter in (False, True):
        b = b"ab\\ncd" if starter else b"abmncd"
        yield Doc("closing quote is byte 0, starter %s" % starter,
                  place_doc(3 * UNIT + 100, [(3, b'"e\\t"'), (2 * UNIT - 1 - len(b), b'"' + b + b'"'), (2 * UNIT + 50, b'"t"')]),
                  False, True, ("close0", starter))
        yield Doc("opening quote is byte 4095, starter %s" % starter,
                  place_doc(3 * UNIT + 100, [(3, b'"e\\t"'), (2 * UNIT - 1, b'"' + b + b'"'), (2 * UNIT + 50, b'"t"')]),
                  False, True, ("open4095", starter))


BIG_STRIDE = 12 * UNIT  # a whole number of blocks per copy: every seam keeps its class


def big_doc():
    """(e) above 4 MiB (the synchronous parse path): rotation documents 0, 1, ... one after the other as the elements of
    one array, each at a multiple of twelve units, so that every hazard stays on its seam"""
    n = (4 << 20) // BIG_STRIDE + 2
    a = bytearray(b" " * (n * BIG_STRIDE))
    for k in range(n):
        d = bytearray(rotation_doc(k, False).data)
        d[0], d[-1] = 0x20, 0x2C
        a[k * BIG_STRIDE:k * BIG_STRIDE + len(d)] = d
    del a[(n - 1) * BIG_STRIDE + ROT_LENGTH:]
    a[0], a[-1] = 0x5B, 0x5D
    return Doc("rotation documents in one array, %d bytes" % len(a), bytes(a), False, True, n)
