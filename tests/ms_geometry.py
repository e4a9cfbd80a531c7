"""Where the MarshalJSON tile walk (k_ms_tile and its helpers, csrc/marshal.hip, behind sjhip_marshal_json) cuts its work,
documents that put an entry exactly on those cuts, and the text every entry must come out as.  No GPU import, no oracle import.

A document is built from a list of ENTRIES -- ("[",) ("{",) ("]",) ("}",) ("key", bytes) ("str", bytes) ("int", v) ("uint", v)
("float", x) ("true",) ("false",) ("null",) ("rec",) (a record break: closing root + opening root) -- and the builder derives
  * the tape word of every entry: the opening root on word 0, one word for brackets, literals and roots, two for strings and
    numbers, the closing root last;
  * the text piece of every entry: its bytes plus ',' (a completed value that is not followed by a closing bracket / root), ':'
    (a key) or nothing; '\\n' for a closing root that is not the last word;
  * the whole MarshalJSON text (the pieces joined) and the source (the same, floats spelled by repr instead of appendFloat).
Float text is number_cases.go_format, integer text str(v), string text escape() below.  Placement is exact: fill() pads with
entries whose width the builder knows ("1," two words, "null," one) and raises when the target lies behind the cursor.

The kernel's cuts (see the issue list in tests/test_ms_geometry.py, which pins every constant here to the source text):
tiles of TILE words, ITEMS words per thread with a two-word look-ahead and a vector load when base + 10 <= n; the anchor in
front of a tile from the REACH words in front of it, else from the global scan; the LDS window of the variant (a tile whose text
is one byte larger writes straight to memory); text shifted together in 8-byte slots; four queues of QCAP slots in two arrays,
thread t owning slots t, t + 256, ...; strings from MS_LONG bytes on taken by a whole wave, LONG_STEP bytes per step; a STAGE
of Strings.B in LDS; LOOKBACK descriptors per step of the single pass; key tiles of KEY_TILE tokens, KEY_ITEMS per thread."""
import collections
import random
import struct

import numpy as np

from number_cases import go_format

TILE = 2048
ITEMS = 8
THREADS = 256
MS_LONG = 64
QCAP = 1024
LONG_STEP = 512
REACH = 64        # words in front of a tile the local anchor search looks at
LOOKBACK = 64     # descriptors per step of the single pass's look-back
KEY_TILE = 4096
KEY_ITEMS = 16
# SJHIP_MS_VARIANT -> (window bytes, stage bytes); "default": chosen per launch by default_form()
VARIANTS = {0: (32768, 0), 3: (16384, 0), 5: (19456, 0), 6: (21504, 0), 7: (13312, 8192)}
WINDOWS = (13312, 16384, 19456, 21504, 32768)
STAGE = 8192
STAGE_HEAD = 24   # a head is taken from the stage only if off - st_base + 24 <= st_avail
STAGED_MAX_STRINGS_PER_TILE = 7168
STAGED_MAX_MSG_PER_TILE = 11264

Doc = collections.namedtuple("Doc", "name data nd info kinds words pieces text soffs toks srcoffs")

CLOSERS = ("]", "}", "rec", "R", "end")
TWO_WORD = ("key", "str", "int", "uint", "float")
TAG = {"[": "[", "{": "{", "]": "]", "}": "}", "key": '"', "str": '"', "int": "l", "uint": "u", "float": "d", "true": "t",
       "false": "f", "null": "n", "r": "r", "R": "r"}

_ESC = {0x22: b'\\"', 0x5C: b"\\\\", 8: b"\\b", 12: b"\\f", 10: b"\\n", 13: b"\\r", 9: b"\\t"}


def escape(s):
    """escapeBytes of the reference's writer: \\" \\\\ \\b \\f \\n \\r \\t, \\u00xx (lowercase) below 0x20, the rest as is"""
    out = bytearray()
    for c in s:
        if c in _ESC:
            out += _ESC[c]
        elif c < 0x20:
            out += b"\\u%04x" % c
        else:
            out.append(c)
    return bytes(out)


def _body(e):
    """(text bytes, source bytes) of an entry without its separator"""
    k = e[0]
    if k in ("key", "str"):
        t = b'"' + escape(e[1]) + b'"'
        return t, t
    if k in ("int", "uint"):
        assert (-(1 << 63) <= e[1] < (1 << 63)) if k == "int" else ((1 << 63) <= e[1] < (1 << 64)), e
        t = str(e[1]).encode()
        return t, t
    if k == "float":
        return go_format(e[1]).encode(), repr(e[1]).encode()
    if k == "rec":
        return b"\n", b"\n"
    t = k.encode()
    return t, t


def _sep(prev, nxt):
    """the separator behind an entry of kind `prev` when an entry of kind `nxt` follows"""
    if prev in (None, "[", "{", "rec"):
        return b""
    if prev == "key":
        return b":"
    return b"" if nxt in CLOSERS else b","


class Builder:
    def __init__(self, nd=False):
        self.nd = nd
        self.ents = []
        self.word = 1        # tape word of the next entry (word 0: the opening root)
        self.text = 0        # text bytes of everything added, without the separator of the last entry
        self.prev = None
        self.tile_text0 = {0: 0}  # text offset of the first entry of every tile

    def next_offset(self, kind):
        """text offset of the next entry if it is of `kind`"""
        return self.text + len(_sep(self.prev, kind))

    def next_rel(self, kind):
        """... relative to the text of the tile its tag word lies in"""
        off = self.next_offset(kind)
        return off - self.tile_text0.get(self.word // TILE, off)

    def add(self, *e):
        kind = e[0]
        off = self.next_offset(kind)
        self.tile_text0.setdefault(self.word // TILE, off)
        self.ents.append(e)
        self.text = off + len(_body(e)[0])
        if kind == "rec":
            self.tile_text0.setdefault((self.word + 1) // TILE, self.text)
        self.word += 2 if kind in TWO_WORD or kind == "rec" else 1
        self.prev = kind
        return len(self.ents) - 1

    def extend(self, ents):
        return [self.add(*e) for e in ents]

    def fill(self, word):
        """pad (inside an array) so that the next entry lies on tape word `word`"""
        if word < self.word:
            raise ValueError(("does not fit", word, self.word))
        if (word - self.word) & 1:
            self.add("null")
        while self.word < word:
            self.add("int", 1)

    def room(self, words):
        """the next `words` words in one tile: pad to the next tile when they would not be"""
        if self.word // TILE != (self.word + words) // TILE:
            self.fill((self.word // TILE + 1) * TILE)

    def align(self, o, kind="str"):
        """a filler string (0..7 bytes) so that the next entry, of `kind`, starts at tile text offset o mod 8"""
        self.add("str", b"")
        n = (o - self.next_rel(kind)) % 8
        self.ents[-1] = ("str", b"fillers"[:n])
        self.text += n

    def finish(self, name, info=None):
        kinds, words, pieces, src, soffs, toks = ["r"], [0], [b""], [b""], [-1], [-1]
        w, so, tok = 1, 0, 0
        for i, e in enumerate(self.ents):
            k = e[0]
            nxt = self.ents[i + 1][0] if i + 1 < len(self.ents) else "end"
            if k == "rec":
                kinds += ["R", "r"]
                words += [w, w + 1]
                pieces += [b"\n", b""]
                src += [b"\n", b""]
                soffs += [-1, -1]
                toks += [-1, -1]
                tok += 1  # (the newline between two records is a token of the structural index)
                w += 2
                continue
            t, s = _body(e)
            sep = _sep(k, nxt)
            kinds.append(k)
            words.append(w)
            pieces.append(t + sep)
            src.append(s + sep)
            toks.append(tok)
            tok += 1 + len(sep)
            if k in ("key", "str"):
                soffs.append(so)
                so += len(e[1])
            else:
                soffs.append(-1)
            w += 2 if k in TWO_WORD else 1
        kinds.append("R")
        words.append(w)
        pieces.append(b"")
        src.append(b"")
        soffs.append(-1)
        toks.append(-1)
        assert w == self.word
        srcoffs = np.concatenate(([0], np.cumsum([len(s) for s in src])))[:-1]
        return Doc(name, b"".join(src), self.nd, info, kinds, np.array(words, dtype=np.int64), pieces, b"".join(pieces),
                   np.array(soffs, dtype=np.int64), np.array(toks, dtype=np.int64), srcoffs)


def build(name, ents, nd=False, info=None):
    b = Builder(nd)
    b.extend(ents)
    return b.finish(name, info)


# ---- what the documents claim, computed from their layout ------------------------------------------------------------------
def n_words(d):
    return int(d.words[-1]) + 1


def n_tiles(d):
    return (n_words(d) + TILE - 1) // TILE


def text_starts(d):
    """text offset of every entry"""
    return np.concatenate(([0], np.cumsum([len(p) for p in d.pieces])))[:-1]


def tile_text_bytes(d):
    """text bytes every tile owns: the pieces of the entries whose tag word lies in it"""
    lens = np.array([len(p) for p in d.pieces], dtype=np.int64)
    return np.bincount(d.words // TILE, weights=lens, minlength=n_tiles(d)).astype(np.int64)


def tile_rel_offsets(d):
    """text offset of every entry inside its tile's text (the offset the window sees)"""
    st = text_starts(d)
    first = np.searchsorted(d.words // TILE, np.arange(n_tiles(d)))  # (every tile holds a tag word: entries are two words at most)
    return st - st[first][d.words // TILE]


def owner(d, k):
    """the entry that owns text byte k -> (tile, tape word, kind, index of the entry)"""
    i = int(np.searchsorted(text_starts(d), k, side="right")) - 1
    while i + 1 < len(d.pieces) and not d.pieces[i]:
        i += 1
    return int(d.words[i]) // TILE, int(d.words[i]), d.kinds[i], i


def default_form(strings_len, msg_len, tiles):
    """launch_ms_tile without SJHIP_MS_VARIANT: -> (window, stage)"""
    if tiles and strings_len // tiles <= STAGED_MAX_STRINGS_PER_TILE and msg_len // tiles <= STAGED_MAX_MSG_PER_TILE:
        return 13312, STAGE
    return 21504, 0


def stage_ranges(d, stage=STAGE):
    """per tile of a copying parse: (st_base, st_avail, [(entry index, off - st_base + 24 - st_avail) of its short strings])"""
    total = d.info["strings_len"]
    out = {}
    for i, k in enumerate(d.kinds):
        if k in ("key", "str") and d.info["slen"][i] < MS_LONG:
            out.setdefault(int(d.words[i]) // TILE, []).append(i)
    res = {}
    for t, idx in out.items():
        lo = min(int(d.soffs[i]) for i in idx)
        base = lo & ~15
        left = total - base
        avail = (left & ~15) if left < stage else stage
        res[t] = (base, avail, lo, [(i, int(d.soffs[i]) - base + STAGE_HEAD - avail) for i in idx])
    return res


# ---- a. tile and thread edges ------------------------------------------------------------------------------------------------
_SAMPLE = {"str": ("str", b"ed\tge"), "int": ("int", -12345), "uint": ("uint", (1 << 63) + 5), "float": ("float", -2.5e-7),
           "true": ("true",), "false": ("false",), "null": ("null",)}
VALUE_KINDS = tuple(_SAMPLE)
A_KINDS = VALUE_KINDS + ("key", "[", "{", "]", "}")
A_POS = (1, 2)  # the tag on the last word in front of the edge (a two-word entry: its raw word behind it), on the second-to-last


def a_sequence(kind, follow):
    """entries that put an entry of `kind` in front of one that closes / does not -> (entries, index of the entry, words in front)"""
    if kind in VALUE_KINDS:
        return ([("[",), _SAMPLE[kind], ("]",)], 1, 1) if follow == "closes" else ([_SAMPLE[kind], ("int", 7)], 0, 0)
    if kind == "key":
        return [("{",), ("key", b"k\"y"), ("int", 8), ("}",)], 1, 1
    if kind == "[":
        return ([("[",), ("]",)], 0, 0) if follow == "closes" else ([("[",), ("true",), ("]",)], 0, 0)
    if kind == "{":
        return ([("{",), ("}",)], 0, 0) if follow == "closes" else ([("{",), ("key", b"q"), ("null",), ("}",)], 0, 0)
    o, c = ("[", "]") if kind == "]" else ("{", "}")
    return ([("[",), (o,), (c,), ("]",)], 2, 2) if follow == "closes" else ([(o,), (c,), ("int", 9)], 1, 1)


def a_cases(nd):
    """(kind, pos, follow): a key is always followed by its value; a root by the next record's value"""
    out = [(k, p, f) for k in A_KINDS for p in A_POS for f in ("closes", "not") if not (k == "key" and f == "closes")]
    if nd:
        out += [(k, p, "not") for k in ("R", "r") for p in A_POS]
    return out


def a_edges(cls):
    """the edges a case document uses, one per case: tile edges, or thread edges that are no tile edge"""
    i = 0
    while True:
        i += 1
        yield TILE * i if cls == "tile" else ITEMS * 3 * i + (ITEMS if (ITEMS * 3 * i) % TILE == 0 else 0)


def a_doc(cls, nd):
    b = Builder(nd)
    b.add("[")
    lay = []
    for (kind, pos, follow), edge in zip(a_cases(nd), a_edges(cls)):
        if kind in ("R", "r"):
            b.fill(edge - pos - (1 if kind == "R" else 2))
            b.extend([("]",), ("rec",), ("[",)])
        else:
            ents, _, front = a_sequence(kind, follow)
            b.fill(edge - pos - front)
            b.extend(ents)
        lay.append((kind, pos, follow, edge))
    b.fill(b.word + 5)
    b.add("]")
    return b.finish("a %s edges%s" % (cls, " nd" if nd else ""), {"family": "a", "edge": cls, "lay": lay})


def a_observed(d, cls):
    """(kind, pos, follow) of every entry whose tag lies on the last / second-to-last word in front of an edge of class `cls`"""
    out = set()
    for i, (k, w) in enumerate(zip(d.kinds[:-1], d.words[:-1])):
        for pos in A_POS:
            e = int(w) + pos
            if e % TILE == 0 if cls == "tile" else (e % ITEMS == 0 and e % TILE != 0):
                out.add((k, pos, "closes" if d.kinds[i + 1] in CLOSERS else "not"))
    return out


A_RESIDUES = (0, 1, 2, 3, 9, 10, 11)


def a_length_docs():
    """tapes of n words, n = 0 1 2 3 9 10 11 mod TILE (n = 1: the last tile holds the closing root only and owns no text; 9, 10,
    11: the last thread around the vector load's `base + 10 <= n`) and n < 10; a string is the last entry"""
    for n in [TILE * 2 + r for r in A_RESIDUES] + [TILE + r for r in A_RESIDUES if r] + [TILE]:
        b = Builder()
        b.add("[")
        b.fill(n - 4)
        b.extend([("str", b"la\\st"), ("]",)])
        yield b.finish("a n=%d" % n, {"family": "a", "n": n})
    yield build("a n=4 object", [("{",), ("}",)], info={"family": "a", "n": 4})  # (the parser takes no scalar as a document: n >= 4)
    for n in range(4, 10):
        b = Builder()
        b.add("[")
        b.fill(n - 2)
        b.add("]")
        yield b.finish("a n=%d" % n, {"family": "a", "n": n})


def a_small_records_doc(records=TILE // 2 + 3):
    """ND records of four words, tiling exactly -- closing root on word 2047, opening root on 2048.  (The parser takes no scalar
    as a record: the four-word records are empty containers.)"""
    b = Builder(True)
    for i in range(records):
        if i:
            b.add("rec")
        b.extend([("[",), ("]",)] if i % 3 else [("{",), ("}",)])
    return b.finish("a nd four-word records", {"family": "a", "records": records})


def family_a():
    for cls in ("tile", "thread"):
        for nd in (False, True):
            yield a_doc(cls, nd)
    yield from a_length_docs()
    yield a_small_records_doc()


# ---- b. anchors ------------------------------------------------------------------------------------------------------------------
TWO_WORD_TOPS = (0x22, 0x6C, 0x75, 0x64)  # " l u d
ONE_WORD_TOPS = tuple(b"{[}]tfnr") + (0x00, 0xFF)
B_RUNS = (31, 32, 33)


def number_with_top(top, i, as_float):
    """an entry whose raw word has the top byte `top`"""
    bits = (top << 56) | (0x0123456789ABCD + 977 * i)
    if as_float:
        assert top not in (0x7F, 0xFF) or (bits >> 52) & 0x7FF != 0x7FF
        return ("float", struct.unpack("<d", struct.pack("<Q", bits))[0])
    return ("int", bits - (1 << 64) if bits >> 63 else bits)


def b_distance(run, parity):
    """words from the anchor to the edge for a run of `run` entries: parity 0 -- the edge behind the run's last raw word;
    parity 1 -- between the last entry's tag and raw word.  Up to REACH the tile finds the anchor itself (REACH: the farthest
    word it sees), beyond it the launch is repeated with the global anchors."""
    return 2 * run + 1 - parity


def b_run_doc(run, parity, edge_tile):
    b = Builder()
    b.add("[")
    edge = edge_tile * TILE
    anchor = edge - b_distance(run, parity)
    b.fill(anchor)
    b.add("null")  # the anchor: the closest word in front of the edge that is no two-word tag
    for i in range(run + 2):  # (the run goes on behind the edge)
        b.add(*number_with_top(TWO_WORD_TOPS[i % 4], i, i % 3 != 0))
    b.extend([("str", b"behind"), ("{",), ("key", b"k"), ("[",), ("int", 1), ("]",), ("}",)])
    b.fill(2 * TILE + 40)
    b.add("]")
    return b.finish("b run %d parity %d edge %d" % (run, parity, edge),
                    {"family": "b", "run": run, "parity": parity, "edge": edge, "anchor": anchor, "local": edge - anchor <= REACH})


def b_top_doc():
    """raw words whose top byte is a one-word tag (or 0x00 / 0xff) as the last word in front of a tile edge and as the first
    word of a tile: anchors by the parity rule, never entries"""
    b = Builder()
    b.add("[")
    lay = []
    t = 1
    for top in ONE_WORD_TOPS:
        for side in ("front", "first"):
            for as_float in ((False, True) if top != 0x00 else (False,)):
                b.fill(t * TILE - (2 if side == "front" else 1))
                b.add(*number_with_top(top, t, as_float))
                lay.append((top, side, t * TILE))
                t += 1
    b.fill(b.word + 3)
    b.add("]")
    return b.finish("b one-word tops", {"family": "b", "lay": lay})


def b_observed_tops(d, tape):
    """(top byte, side) of the raw words around every tile edge, from a tape"""
    out = set()
    for i, (k, w) in enumerate(zip(d.kinds, d.words)):
        if k in ("int", "uint", "float"):
            raw = int(w) + 1
            if (raw + 1) % TILE == 0:
                out.add((int(tape[raw]) >> 56, "front"))
            if raw % TILE == 0:
                out.add((int(tape[raw]) >> 56, "first"))
    return out


def family_b():
    for run in B_RUNS:
        for parity in (0, 1):
            for edge_tile in (1, 2):
                yield b_run_doc(run, parity, edge_tile)
    yield b_top_doc()


# ---- c. window edges -----------------------------------------------------------------------------------------------------------
_EVERY_KIND = [("{",), ("key", b"a\nb"), ("[",), ("true",), ("false",), ("null",), ("int", -(1 << 63)), ("uint", (1 << 64) - 1),
               ("float", 1e21), ("float", 5e-324), ("str", b""), ("str", b"x" * 70 + b'"' + b"y" * 600), ("]",), ("key", b"o"),
               ("{",), ("}",), ("}",)]


C_TAIL = 16000


def _c_build(window, delta, lens, pad):
    b = Builder()
    b.add("[")
    b.fill(TILE)
    b.extend(_EVERY_KIND)
    for i, n in enumerate(lens):
        b.add("str", ((b"%d " % i) * n)[:n])
    b.add("str", b"p" * pad)
    b.fill(2 * TILE)
    # (the default launch takes the window of 21504 bytes only for a tape with much text per tile: C_TAIL bytes more in tile 2)
    b.extend([("str", b"tail" * (C_TAIL // 4 if window == 21504 else 1)), ("int", 3), ("]",)])
    return b.finish("c window %d%+d" % (window, delta), {"family": "c", "window": window, "delta": delta, "tile": 1,
                                                         "tile_text": window + delta})


def c_doc(window, delta):
    """three tiles, the middle one holds every entry kind and exactly window + delta bytes of text: strings of one short length
    in place of "1," fillers, 40-byte ones for most of the rest and one padding string for the last bytes"""
    target = window + delta
    size = max(20, (target - int(tile_text_bytes(_c_build(window, delta, [], 0))[1])) // 900 + 1)
    lens = []
    while True:
        left = target - int(tile_text_bytes(_c_build(window, delta, lens, 0))[1])
        if left < MS_LONG:
            break
        step = size if left >= 3 * (size + 1) else 40 if left > 100 else left - 50
        lens += [step] * max(1, left // (step + 1) - 2 if step == size else 1)
    if left < 0:
        raise ValueError(("does not fit", window, delta, left))
    return _c_build(window, delta, lens, left)


def c_short_only_doc(n_false, n_float):
    """a middle tile over the window that holds only short entries: literals and numbers written straight to memory"""
    assert n_false + 2 * n_float == TILE
    b = Builder()
    b.add("[")
    b.fill(TILE)
    rnd = random.Random(n_false)
    for i in range(max(n_false, n_float)):
        if i < n_false:
            b.add("false")
        if i < n_float:
            b.add("float", -(1.0 + rnd.random()) * 10.0 ** -(100 + i % 150))
    assert b.word == 2 * TILE
    b.extend([("int", 5), ("]",)])
    d = b.finish("c short entries only %d/%d" % (n_false, n_float), {"family": "c", "tile": 1})
    d.info["tile_text"] = int(tile_text_bytes(d)[1])
    return d


def family_c():
    for w in WINDOWS:
        for delta in (-1, 0, 1):
            yield c_doc(w, delta)
    yield c_short_only_doc(1022, 513)
    yield c_short_only_doc(400, 824)


# ---- d. slot alignment ---------------------------------------------------------------------------------------------------------
D_LENGTHS = tuple(range(0, 18)) + (23, 24, 25, 31, 32, 33) + tuple(range(55, 64))
D_ESCAPED = (0x22, 0x5C, 0x0A, 0x01)
D_FORMS = ("value,", "value", "key")
D_LONG_LENGTHS = (64, 65, 511, 512, 513, 1023, 1024, 1025, 4096 + 3)
D_LONG_ESCAPES = (7, 8, 511, 512, "last")
D_TILE_TEXT = 10000  # a tile of the fitting documents is padded out with "1," once it holds this much text


def _d_string(n, esc=()):
    s = bytearray((0x41 + i % 26) for i in range(n))
    for p, c in esc:
        s[p] = c
    return bytes(s)


def _d_keep_fitting(b):
    t = b.word // TILE
    if b.text - b.tile_text0.get(t, b.text) > D_TILE_TEXT:
        b.fill((t + 1) * TILE)


def _d_put(b, o, form, s, words=12, fit=True):
    if fit:
        _d_keep_fitting(b)
    b.room(words)
    if form == "key":
        b.align((o - 1) % 8, "{")
        b.extend([("{",), ("key", s), ("int", 0), ("}",)])
    elif form == "value":
        b.align((o - 1) % 8, "[")
        b.extend([("[",), ("str", s), ("]",)])
    else:
        b.align(o, "str")
        b.add("str", s)


def d_short_docs():
    """(clean) every length x offset x form; (one) one escaped byte at every position, the escaped byte and the form in
    rotation; (three) escaped bytes at positions 7, 8 and 9 together"""
    for name in ("clean", "one", "three"):
        b = Builder()
        b.add("[")
        for n in D_LENGTHS:
            for o in range(8):
                if name == "clean":
                    for form in D_FORMS:
                        _d_put(b, o, form, _d_string(n))
                elif name == "one":
                    for p in range(n):
                        _d_put(b, o, D_FORMS[(o + p) % 3], _d_string(n, [(p, D_ESCAPED[(o + p + n) % 4])]))
                elif n >= 10:
                    for r in range(3):
                        _d_put(b, o, D_FORMS[r], _d_string(n, [(7 + j, D_ESCAPED[(o + j + r) % 4]) for j in range(3)]))
        b.add("]")
        yield b.finish("d short strings, %s" % name, {"family": "d", "part": name})


def d_other_doc():
    """every literal and bracket at every offset, integers and floats with the ',' behind them, a run of closing roots"""
    b = Builder(True)
    b.add("[")
    for o in range(8):
        for e in (("true",), ("false",), ("null",), ("int", -98765432101), ("uint", (1 << 63) + o), ("float", 1.5e300), ("int", o)):
            b.room(8)
            b.align(o, e[0])
            b.add(*e)
        for br in ("[", "{"):
            b.room(8)
            b.align(o, br)
            b.extend([(br,), ("]" if br == "[" else "}",)])
            b.room(8)
            b.align((o - 1) % 8, br)  # ... and the closing bracket at o
            b.extend([(br,), ("]" if br == "[" else "}",)])
        b.room(40)
        b.align((o - 1) % 8, "]")  # '\n' pieces at o, o + 3, ...: "]\n" + "[]\n" * 8 + "["
        b.add("]")
        for i in range(8):
            b.extend([("rec",), ("[",), ("]",)] if i % 2 else [("rec",), ("{",), ("}",)])
        b.extend([("rec",), ("[",)])
    b.add("]")
    return b.finish("d literals, brackets, numbers, roots", {"family": "d", "part": "other"})


def d_long_cases():
    for n in D_LONG_LENGTHS:
        yield n, None
        for p in D_LONG_ESCAPES:
            q = n - 1 if p == "last" else p
            if q < n:
                yield n, q


def d_long_doc(fits):
    """long strings at every offset, clean and with one escaped byte; fits: every tile's text stays inside the smallest window;
    else every tile holds one string larger than the largest window"""
    b = Builder()
    b.add("[")
    for o in range(8):
        for j, (n, q) in enumerate(d_long_cases()):
            s = _d_string(n, [] if q is None else [(q, D_ESCAPED[(o + j) % 4])])
            t = b.word // TILE
            if fits and b.text - b.tile_text0.get(t, b.text) + n > D_TILE_TEXT:
                b.fill((t + 1) * TILE)
            _d_put(b, o, D_FORMS[(o + j) % 3], s, fit=False)
        if not fits:
            b.add("str", b"w" * 33000)
            b.fill((b.word // TILE + 1) * TILE)
    b.add("]")
    return b.finish("d long strings, %s" % ("fitting tiles" if fits else "tiles over the window"),
                    {"family": "d", "part": "long", "fits": fits})


def d_observed(d, lo=0, hi=1 << 30):
    """(offset mod 8, length, escaped positions) of every string entry with lo <= length < hi, from the entries' bytes"""
    rel = tile_rel_offsets(d)
    out = set()
    for i, k in enumerate(d.kinds):
        if k in ("key", "str"):
            s = d.info["_bytes"][i]
            if lo <= len(s) < hi:
                out.add((int(rel[i]) % 8, len(s), tuple(p for p, c in enumerate(s) if c in D_ESCAPED), k,
                         d.pieces[i][-1:] in (b",", b":")))
    return out


def family_d():
    yield from d_short_docs()
    yield d_other_doc()
    yield d_long_doc(True)
    yield d_long_doc(False)


# ---- e. queues -------------------------------------------------------------------------------------------------------------------
def _e_entry(kind, i):
    if kind == "empty":
        return ("str", b"")
    if kind == "one":
        return ("str", bytes([0x61 + i % 26]))
    if kind == "short":
        return ("str", b"s%d" % i)
    if kind == "long":
        return ("str", _d_string(MS_LONG, [(i % MS_LONG, 0x0A)] if i % 5 == 0 else []))
    if kind == "int":
        return ("int", (i * 7919) * (-1 if i % 2 else 1))
    return ("float", (i + 1) * 0.001)


def e_doc(name, kinds_of_tile1):
    """tile 0: '[' and 1023 two-word entries; tile 1: the 1024 entries `kinds_of_tile1` names, exactly"""
    assert len(kinds_of_tile1) == QCAP
    b = Builder()
    b.add("[")
    for i in range(QCAP - 1):
        b.add(*_e_entry(("short", "int", "float")[i % 3], i))
    assert b.word == TILE
    for i, k in enumerate(kinds_of_tile1):
        b.add(*_e_entry(k, i))
    assert b.word == 2 * TILE
    b.add("]")
    return b.finish("e " + name, {"family": "e", "tile": 1})


def _e_mix(a, na, b, nb, rest="int"):
    """na entries of kind a and nb of kind b spread evenly over QCAP entries, the rest `rest`"""
    out = [rest] * QCAP
    for j in range(na):
        out[j * QCAP // max(na, 1)] = a
    free = [i for i, k in enumerate(out) if k == rest]
    for j in range(nb):
        out[free[j * len(free) // max(nb, 1)]] = b
    return out


E_FULL = ("empty", "one", "long", "int", "float")
E_SPLITS = ((1, 1023), (512, 512), (1023, 1))
E_SHORT_COUNTS = (255, 256, 257, 767, 768, 769, 1023)
E_LONG_COUNTS = (3, 4, 5)


def e_object_doc(key_last):
    """strings only, half of them keys; ordinal 1023 of tile 1 is a key (key_last) or a value"""
    b = Builder()
    if key_last:
        b.add("{")      # word 1: tile 0 ends behind a key, tile 1 starts with its value
    else:
        b.extend([("[",), ("null",), ("{",)])  # tile 1 starts with a key
    i = 0
    while b.word < 2 * TILE:
        b.add("key" if i % 2 == 0 else "str", b"%c%d" % (0x6B if i % 2 == 0 else 0x76, i))
        i += 1
    assert b.word == 2 * TILE and (i % 2 == 1) == key_last
    if key_last:
        b.extend([("str", b"v"), ("}",)])
    else:
        b.extend([("}",), ("]",)])
    return b.finish("e object, ordinal 1023 a %s" % ("key" if key_last else "value"), {"family": "e", "tile": 1, "key_last": key_last})


def e_observed(d, tile=1):
    """(short strings, long strings, integers, floats) whose tag word lies in `tile`"""
    c = [0, 0, 0, 0]
    for i, (k, w) in enumerate(zip(d.kinds, d.words)):
        if int(w) // TILE == tile:
            if k in ("key", "str"):
                c[1 if len(d.info["_bytes"][i]) >= MS_LONG else 0] += 1
            elif k in ("int", "uint"):
                c[2] += 1
            elif k == "float":
                c[3] += 1
    return tuple(c)


def family_e():
    for k in E_FULL:
        yield e_doc("1024 x %s" % k, [k] * QCAP)
    for a, b_ in E_SPLITS:
        yield e_doc("short/long %d/%d" % (a, b_), _e_mix("short", a, "long", b_))
        yield e_doc("int/float %d/%d" % (a, b_), _e_mix("int", a, "float", b_))
    for n in E_SHORT_COUNTS:
        yield e_doc("%d short strings" % n, _e_mix("short", n, "long", 0))
    for n in E_LONG_COUNTS:
        yield e_doc("%d long strings" % n, _e_mix("long", n, "short", 0, rest="float"))
    yield e_object_doc(True)
    yield e_object_doc(False)


# ---- f. stage and buffer ends (copy mode, the staged form of the default launch) -------------------------------------------------------
F_LO_MOD16 = (0, 1, 15, 16)
F_DISTANCES = (-1, 0, 1)


def f_lo_doc(lo):
    """the lowest short-string offset of tile 1 at `lo` mod 16 (16: one aligned block further)"""
    b = Builder()
    b.add("[")
    b.add("str", b"h" * (160 + lo))
    b.fill(TILE)
    for i in range(40):
        b.add("str", b"%c%s" % (0x61 + i % 26, b"z" * (i % 23)))
    b.add("]")
    return b.finish("f lowest offset %d mod 16" % lo, {"family": "f", "lo": lo})


def f_distance_doc(cut):
    """tiles 1, 2, 3: a 16-byte string whose off - st_base + 24 is st_avail - 1, st_avail, st_avail + 1; cut: st_avail is what the
    end of Strings.B leaves (tile t of three-tile documents, one per distance), else the full stage"""
    docs = []
    for dist in F_DISTANCES:
        b = Builder()
        b.add("[")
        b.fill(TILE)
        lead = 5  # tile 1's lowest string starts at Strings.B offset 5 + what tile 0 holds (nothing): st_base = 0
        b.add("str", b"L" * lead)
        if cut:
            avail = 1024
            at = avail - STAGE_HEAD + dist  # Strings.B offset of the string under test
        else:
            avail = STAGE
            at = avail - STAGE_HEAD + dist
        have = lead
        i = 0
        while at - have > 60:
            b.add("str", bytes([0x30 + i % 10]) * 60)
            have += 60
            i += 1
        b.add("str", b"m" * (at - have))
        b.add("str", b"0123456789\tbcdef")  # 16 bytes at `at`
        end = at + 16
        if cut:
            total = avail + 9   # Strings.B ends 9 bytes behind the last whole 16-byte block
            b.add("str", b"e" * (total - end))
        else:
            b.add("str", b"beyond the stage " * 3)
        b.add("]")
        docs.append(b.finish("f distance %+d, %s" % (dist, "cut stage" if cut else "full stage"),
                             {"family": "f", "dist": dist, "cut": cut, "tile": 1}))
    return docs


def f_tail_docs():
    """the last string of Strings.B (and of the message) 1 .. 16 bytes long, its last byte two bytes in front of the message's end
    (one byte is not possible: the parser takes no scalar as a document, a document ends with a closing bracket)"""
    for n in range(1, 17):
        s = b"0123456789abcdef"[:n]
        yield build("f last string %d bytes, array" % n, [("[",), ("str", b"first\n"), ("int", n), ("str", s), ("]",)],
                    info={"family": "f", "tail": n, "end": 2})


def f_straddle_doc():
    """short strings on both sides of a long one: the strings behind it lie beyond the staged range"""
    b = Builder()
    b.add("[")
    b.fill(TILE)
    for i in range(30):
        b.add("str", b"front %d" % i)
    b.add("str", b"L" * 20000)
    for i in range(300):
        b.add("str", b"behind\t%d" % i)
    b.fill(5 * TILE)  # (words enough for the default launch to keep the staged form)
    b.add("]")
    return b.finish("f short strings around a long one", {"family": "f", "straddle": True})


def family_f():
    for lo in F_LO_MOD16:
        yield f_lo_doc(lo)
    yield from f_distance_doc(False)
    yield from f_distance_doc(True)
    yield from f_tail_docs()
    yield f_straddle_doc()


# ---- g. look-back and tile counts -----------------------------------------------------------------------------------------------
G_TILES = (1, 2, 63, 64, 65, 66, 128, 129, 130)
G_FORMS = ("plain", "over", "zero")


def g_doc(tiles, form="plain"):
    """`tiles` tiles at about two text bytes per word; over: every 7th tile holds a string larger than every window;
    zero: the last tile holds the closing root only"""
    n = tiles * TILE - 700 if form != "zero" else (tiles - 1) * TILE + 1
    pattern = [("int", 3), ("str", b"s"), ("true",), ("{",), ("key", b"k"), ("int", 2), ("}",), ("float", 0.5)]
    b = Builder()
    b.add("[")
    i, over = 0, set()
    while b.word < n - 12 or i % 8 in (4, 5, 6):  # (never stop inside the object)
        t = b.word // TILE
        if form == "over" and t % 7 == 3 and t not in over and i % 8 == 0 and b.word % TILE >= 8:
            b.add("str", b"O" * 33000)
            over.add(t)
        b.add(*pattern[i % 8])
        i += 1
    b.fill(n - 2)
    b.add("]")
    assert b.word + 1 == n
    return b.finish("g %d tiles, %s" % (tiles, form), {"family": "g", "tiles": tiles, "form": form})


def family_g():
    for t in G_TILES:
        yield g_doc(t)
    for t in (65, 129):
        yield g_doc(t, "over")
        yield g_doc(t, "zero")


# ---- h. recovered key flags --------------------------------------------------------------------------------------------------------
def _h_fill_tokens(b, tok, target):
    """ints (two tokens each with their ',') and at most one '[' (one token) until the next entry is token `target`"""
    opened = 0
    if (target - tok) & 1:
        b.add("[")
        tok += 1
        opened = 1
    while tok < target:
        b.add("int", 1)
        tok += 2
    return tok, opened


def h_doc():
    """a key and a value string as token KEY_TILE - 1 of a key tile (its ':' / ',' token 0 of the next) and as token
    KEY_ITEMS - 1 of a thread"""
    b = Builder()
    b.add("[")
    tok, depth, lay = 1, 0, []
    targets = [("key", 5 * KEY_ITEMS + KEY_ITEMS - 1), ("str", 9 * KEY_ITEMS + KEY_ITEMS - 1), ("key", KEY_TILE - 1),
               ("str", 2 * KEY_TILE - 1), ("key", 2 * KEY_TILE + 77 * KEY_ITEMS + KEY_ITEMS - 1), ("str", 3 * KEY_TILE - 1),
               ("key", 4 * KEY_TILE - 1)]
    for kind, target in targets:
        if kind == "key":
            tok, op = _h_fill_tokens(b, tok, target - 1)
            b.extend([("{",), ("key", b"key at %d" % target), ("str", b"v"), ("}",)])
            tok += 1 + 2 + 1 + 2
        else:
            tok, op = _h_fill_tokens(b, tok, target)
            b.add("str", b"value at %d" % target)
            tok += 2
        depth += op
        lay.append((kind, target))
    b.add("int", 0)
    for _ in range(depth + 1):
        b.add("]")
    return b.finish("h key tile and thread edges", {"family": "h", "lay": lay})


def h_last_docs():
    """the last string token next to the end of the token array: only the closing bracket behind it (the parser takes no scalar as
    a document or a record, so a string is never the last token)"""
    yield build("h last string token, array", [("[",), ("str", b"last but one token"), ("]",)], info={"family": "h", "last": True})
    yield build("h last string token, nd", [("{",), ("key", b"a"), ("int", 1), ("}",), ("rec",), ("[",), ("str", b"last record"), ("]",)],
                nd=True, info={"family": "h", "last": True})


def family_h():
    yield h_doc()
    yield from h_last_docs()


# ---- i. the device's number formatting ------------------------------------------------------------------------------------------------
HAND_FLOATS = (1.0, 0.1, 0.5, 1e-6, 9.999999999999999e-7, 1e21, 9.999999999999999e20, 1e22, 1e23, 5e-324, 1.7976931348623157e308,
               123456789.0, 1e15, 1e16, 1e17, 123456789012345680.0, 0.3, 2.5e-8, 1e-7, 1e-10, 4.35, 0.000001, 100.0, 1e20,
               9007199254740993.0, 2.2250738585072014e-308, 2.225073858507201e-308, 8.41e21, 6.02214076e23, 299792458.0)
HAND_BITS = (0, 1 << 63, 1, 2, (1 << 52) - 1, 1 << 52, (1 << 52) + 1, 0x7FEFFFFFFFFFFFFF, 0x0010000000000000, 0x000FFFFFFFFFFFFF)
I_RANDOM = 20000


def i_float_bits():
    rnd = random.Random(20261019)
    bits = list(HAND_BITS)
    for v in HAND_FLOATS:
        x = struct.unpack("<Q", struct.pack("<d", v))[0]
        bits += [x, x | (1 << 63)]
    for e in range(0, 2047):  # every binade: its first, a random and its last value, in both signs
        for m in (0, rnd.getrandbits(52), (1 << 52) - 1):
            bits += [(e << 52) | m, (1 << 63) | (e << 52) | m]
    while len(bits) < len(HAND_BITS) + 2 * len(HAND_FLOATS) + 6 * 2047 + I_RANDOM:
        x = rnd.getrandbits(64)
        if (x >> 52) & 0x7FF != 0x7FF:
            bits.append(x)
    return bits


def i_ints():
    out = []
    for k in range(0, 20):
        for v in (10 ** k - 1, 10 ** k, -(10 ** k - 1), -(10 ** k)):
            if -(1 << 63) <= v < (1 << 64):
                out.append(v)
    return out + [(1 << 63) - 1, -(1 << 63), 1 << 63, (1 << 64) - 1]


def i_float_doc():
    b = Builder()
    b.add("[")
    for x in i_float_bits():
        b.add("float", struct.unpack("<d", struct.pack("<Q", x))[0])
    b.add("]")
    return b.finish("i floats", {"family": "i"})


def i_int_doc():
    b = Builder()
    b.add("[")
    for v in i_ints():
        b.add("uint" if v >= 1 << 63 else "int", v)
    b.add("]")
    return b.finish("i integers", {"family": "i"})


def family_i():
    yield i_float_doc()
    yield i_int_doc()


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e, "f": family_f, "g": family_g, "h": family_h,
            "i": family_i}


def family(name):
    """the documents of a family, every one with the bytes and lengths of its strings by entry index in info"""
    for d in FAMILIES[name]():
        by = {}
        for i, k in enumerate(d.kinds):
            if k in ("key", "str"):
                p = d.pieces[i]
                by[i] = unescape(p[1:p.rindex(b'"')])
        d.info["_bytes"] = by
        d.info["slen"] = {i: len(s) for i, s in by.items()}
        d.info["strings_len"] = sum(len(s) for s in by.values())
        yield d


_UNESC = {v: bytes([k]) for k, v in _ESC.items()}


def unescape(t):
    """escape() backwards"""
    out = bytearray()
    i = 0
    while i < len(t):
        if t[i] != 0x5C:
            out.append(t[i])
            i += 1
        elif t[i + 1] == 0x75:
            out.append(int(t[i + 2:i + 6], 16))
            i += 6
        else:
            out += _UNESC[t[i:i + 2]]
            i += 2
    return bytes(out)
