"""Where Serialize and Deserialize (k_ser_tile, k_des_tile and the launches around them, csrc/serialize.hip) cut their work,
documents that put an entry exactly on those cuts, and the columns and the framed stream every document must come out as.
No GPU import, no oracle import.

Documents are built with the builder of tests/ms_geometry.py (entries in, tape words and Strings.B offsets out); Builder below
only adds source spellings the text builder has no use for (an overflowed integer, which parses to a float whose tag word carries
a flag -- the 'e' entry of the tag column -- and an escaped spelling of a plain string) and placement by tag index.  From the
entries Doc derives, in plain Python:
  * the tape (brackets and roots point at each other, strings carry their Strings.B offset with the buffer bit);
  * the tag column (one byte per entry, 'e' for a flagged float), the value column (string: column offset and length; l u d: the
    value word; e: tag word and value; { [ r: payload - own index mod 2^64, so the closing root wraps; nothing else);
  * the string column: plain (Strings.B itself, the tape's offsets) and de-duplicating (ser_hash mirrored; the first string
    entry of a slot is the one with the smallest tape index; an entry is kept unless it has the length and bytes of that first;
    kept strings in tape order; a dropped entry stores its slot's first string's offset; an empty string stores 0);
  * the framed stream, version 3.
valid_dedup() checks a de-duplicated stream without the hash: it holds for any table policy.  owner() names the tile, thread,
tape word and entry that own a byte of a column.

The kernels' cuts (pinned to the source text by tests/test_ser_geometry.py): Serialize walks tiles of TILE words, ITEMS per
thread with the word behind them as look-ahead, four waves; the anchor of the tag / raw classification comes from the REACH words
in front of a tile, else the launch is repeated with the global anchors; the de-duplication table has 2^SER_SLOT_BITS slots;
Deserialize walks tiles of DS_TILE tags, DS_ITEMS per thread; the per-tile counts of both are scanned by one block of SCAN_WAVES
waves over ranges rounded to SCAN_ROUND."""
import functools
import random
import struct

import numpy as np

import ms_geometry as M

TILE, ITEMS, THREADS, REACH = M.TILE, M.ITEMS, M.THREADS, M.REACH
WAVE_WORDS = 64 * ITEMS
DS_THREADS, DS_ITEMS = 256, 16
DS_TILE = DS_THREADS * DS_ITEMS
SER_SLOT_BITS = 20
HASH_SEED, HASH_MUL, HASH_FIN = 0x9E3779B97F4A7C15, 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53
HASH_SHIFT, HASH_FIN_SHIFT = 29, 31
SCAN_WAVES, SCAN_ROUND = 16, 64
PAYLOAD = (1 << 56) - 1
STRINGBUFBIT = 1 << 55
U64 = (1 << 64) - 1


def scan_per(n):
    """block1024_scan_array: elements per wave"""
    return ((n + SCAN_WAVES - 1) // SCAN_WAVES + SCAN_ROUND - 1) // SCAN_ROUND * SCAN_ROUND


def ser_hash(s):
    """ser_hash of csrc/serialize.hip: 8 bytes at a time, a byte tail, the top SER_SLOT_BITS bits"""
    n = len(s)
    h = HASH_SEED ^ n
    i = 0
    while i + 8 <= n:
        h = (((h ^ int.from_bytes(s[i:i + 8], "little")) * HASH_MUL) + (h >> HASH_SHIFT)) & U64
        i += 8
    h = ((h ^ int.from_bytes(s[i:], "little")) * HASH_FIN) & U64
    return (h ^ (h >> HASH_FIN_SHIFT)) >> (64 - SER_SLOT_BITS)


# ---- the frame ----------------------------------------------------------------------------------------------------------------------
def uvarint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def uvarint_len(v):
    return len(uvarint(v))


def block_len(n):
    return uvarint_len(n) + uvarint_len(n + 1) + 1 + n


def rest_len(tape_len, s, t, v):
    return uvarint_len(tape_len) + 2 + block_len(s) + block_len(t) + block_len(v)


def frame(tape_len, scol, tags, vals, version=3, rest_delta=0, bsize_delta=None, btype=None, sizes=None):
    """version, uvarint(rest), uvarint(tape_len), an empty Strings block, then Message (the string column), tags and values as
    uvarint(len) uvarint(len + 1) 00 data.  The keyword arguments write a corrupt header: (column index, value) each."""
    body = bytearray(uvarint(tape_len) + b"\x00\x00")
    for i, col in enumerate((scol, tags, vals)):
        n, bs = len(col), len(col) + 1
        if sizes and sizes[0] == i:
            n, bs = sizes[1], sizes[2]
        if bsize_delta and bsize_delta[0] == i:
            bs += bsize_delta[1]
        body += uvarint(n) + uvarint(bs) + bytes([btype[1] if btype and btype[0] == i else 0]) + bytes(col)
    return bytes([version]) + uvarint(len(body) + rest_delta) + bytes(body)


def read_uvarint(b, o):
    x = s = 0
    while True:
        c = b[o]
        o += 1
        x |= (c & 0x7F) << s
        s += 7
        if c < 0x80:
            return x, o


def unframe(stream):
    """-> dict: tape_len, rest, the three columns, the stream offset of each, and the offsets of all header bytes"""
    b = bytes(stream)
    assert b[0] == 3
    rest, o = read_uvarint(b, 1)
    assert rest == len(b) - o, (rest, len(b), o)
    tape_len, o = read_uvarint(b, o)
    assert b[o:o + 2] == b"\x00\x00"
    o += 2
    out = {"tape_len": tape_len, "rest": rest, "at": {}}
    header = list(range(o))
    for name in ("strings", "tags", "values"):
        o0 = o
        n, o = read_uvarint(b, o)
        bs, o = read_uvarint(b, o)
        assert bs == n + 1 and b[o] == 0, name
        o += 1
        header += range(o0, o)
        out[name] = b[o:o + n]
        out["at"][name] = o
        o += n
    assert o == len(b)
    out["header"] = header
    return out


# ---- builder and document ---------------------------------------------------------------------------------------------------------------
E_BASE = 123456789012345678901234567890


def e_spelling(i):
    """an integer too large for 64 bits: it parses to a float whose tag word carries the overflow flag"""
    return b"%d" % (E_BASE + i * 10 ** 15)


class Builder(M.Builder):
    """ms_geometry.Builder with source spellings of its own for single entries and with placement by tag index"""

    def __init__(self, nd=False):
        super().__init__(nd)
        self.spell = {}
        self.ntags = 1  # the opening root

    def add(self, *e):
        self.ntags += 2 if e[0] == "rec" else 1
        return super().add(*e)

    def add_e(self, i=0):
        idx = self.add("float", float(int(e_spelling(i))))
        self.spell[idx] = e_spelling(i)
        return idx

    def add_spelled(self, kind, s, src):
        idx = self.add(kind, s)
        self.spell[idx] = src
        return idx

    def put(self, e):
        return self.add_e(e[1]) if e[0] == "e" else self.add_spelled(*e[1:]) if e[0] == "spelled" else self.add(*e)

    def fill_tags(self, tag):
        """pad (inside an array) so that the next entry is tag `tag` of the tag column"""
        if tag < self.ntags:
            raise ValueError(("does not fit", tag, self.ntags))
        while self.ntags < tag:
            self.add("null")

    def done(self, name, info=None):
        return Doc(self, name, info)


class Doc:
    big = False

    def __init__(self, b, name, info):
        d = b.finish(name, info)
        self.name, self.nd, self.info = name, b.nd, dict(info or {})
        self.kinds, self.words = d.kinds, d.words
        self.ents, at = [None], {}
        for j, e in enumerate(b.ents):
            at[j] = len(self.ents)
            self.ents += [None, None] if e[0] == "rec" else [e]
        self.ents.append(None)
        data = d.data
        self.flagged = set()
        if b.spell:
            offs = list(d.srcoffs) + [len(data)]
            pieces = [data[offs[k]:offs[k + 1]] for k in range(len(self.kinds))]
            for j, src in b.spell.items():
                k = at[j]
                natural = M._body(b.ents[j])[1]
                assert pieces[k].startswith(natural)
                pieces[k] = src + pieces[k][len(natural):]
                if b.ents[j][0] == "float":
                    self.flagged.add(k)
            data = b"".join(pieces)
        self.data = data
        self.n = int(self.words[-1]) + 1
        self.strs = [(k, self.ents[k][1]) for k, kd in enumerate(self.kinds) if kd in ("key", "str")]
        self.strings_b = b"".join(s for _, s in self.strs)

    @property
    def tiles(self):
        return (self.n + TILE - 1) // TILE

    @property
    def tag_tiles(self):
        return (len(self.kinds) + DS_TILE - 1) // DS_TILE

    def label(self, k):
        kd = self.kinds[k]
        if kd == "float" and k in self.flagged:
            return "e"
        if kd == "str" and not self.ents[k][1]:
            return "empty"
        if kd == "R" and k == len(self.kinds) - 1:
            return "end"
        return kd

    @functools.cached_property
    def soffs(self):
        out, o = {}, 0
        for k, s in self.strs:
            out[k] = o
            o += len(s)
        return out

    @functools.cached_property
    def tape(self):
        t = [0] * self.n
        soffs, stack, root = self.soffs, [], 0
        for k, (kd, w) in enumerate(zip(self.kinds, self.words.tolist())):
            if kd == "r":
                root = w
            elif kd == "R":
                t[w] = (0x72 << 56) | root
                t[root] = (0x72 << 56) | (w + 1)
            elif kd in ("[", "{"):
                stack.append(w)
            elif kd in ("]", "}"):
                o = stack.pop()
                t[w] = (ord(kd) << 56) | o
                t[o] = ((ord(kd) - 2) << 56) | (w + 1)
            elif kd in ("key", "str"):
                t[w] = (0x22 << 56) | STRINGBUFBIT | soffs[k]
                t[w + 1] = len(self.ents[k][1])
            elif kd in ("int", "uint"):
                t[w] = ord("l" if kd == "int" else "u") << 56
                t[w + 1] = self.ents[k][1] & U64
            elif kd == "float":
                t[w] = (0x64 << 56) | (1 if k in self.flagged else 0)
                t[w + 1] = struct.unpack("<Q", struct.pack("<d", self.ents[k][1]))[0]
            else:
                t[w] = ord(kd[0]) << 56
        assert not stack
        return np.array(t, dtype=np.uint64)

    # -- the string column
    @functools.cached_property
    def plan(self):
        """the kernel's policy -> (kept entries, {dropped entry: the entry whose offset it stores})"""
        first, kept, target = {}, set(), {}
        slots = {k: ser_hash(s) for k, s in self.strs if s}
        for k, s in self.strs:
            if s:
                first.setdefault(slots[k], k)
        for k, s in self.strs:
            if not s:
                continue
            f = first[slots[k]]
            if f == k or self.ents[f][1] != s:
                kept.add(k)
            else:
                target[k] = f
        return kept, target

    def string_column(self, kept, target):
        """-> (column, {entry: stored offset}) for any choice of kept entries and targets"""
        col, off = bytearray(), {}
        for k, s in self.strs:
            if k in kept:
                off[k] = len(col)
                col += s
        for k, s in self.strs:
            if k not in kept:
                off[k] = off[target[k]] if s else 0
        return bytes(col), off

    def columns(self, dedup, plan=None):
        """-> (string column, tag column, value column as a list of words); the entries' value offsets in self.vstart"""
        if dedup or plan:
            scol, off = self.string_column(*(plan or self.plan))
        else:
            scol, off = self.strings_b, self.soffs
        tape = self.tape.tolist()
        tags, vals, vstart = bytearray(), [], []
        for k, (kd, w) in enumerate(zip(self.kinds, self.words.tolist())):
            t = tape[w]
            vstart.append(8 * len(vals))
            if kd in ("key", "str"):
                tags.append(0x22)
                vals += [off[k], len(self.ents[k][1])]
            elif kd in ("int", "uint"):
                tags.append(t >> 56)
                vals.append(tape[w + 1])
            elif kd == "float":
                if t & PAYLOAD:
                    tags.append(0x65)
                    vals += [t, tape[w + 1]]
                else:
                    tags.append(0x64)
                    vals.append(tape[w + 1])
            elif kd in ("{", "[", "r", "R"):
                tags.append(t >> 56)
                vals.append(((t & PAYLOAD) - w) & U64)
            else:
                tags.append(t >> 56)
        self.vstart = vstart
        return scol, bytes(tags), vals

    @functools.lru_cache(maxsize=None)
    def stream(self, dedup):
        scol, tags, vals = self.columns(dedup)
        return frame(self.n, scol, tags, np.array(vals, dtype=np.uint64).tobytes())

    def stream_with(self, plan):
        scol, tags, vals = self.columns(True, plan)
        return frame(self.n, scol, tags, np.array(vals, dtype=np.uint64).tobytes())

    def sizes(self, dedup):
        u = unframe(self.stream(dedup))
        return {"tags": len(u["tags"]), "values": len(u["values"]), "strings": len(u["strings"]), "stream": len(self.stream(dedup))}


class BigDoc:
    """a document built by byte multiplication: compared with the oracle only, never walked here; it holds no string"""
    big = True

    def __init__(self, name, data, info, nd=False):
        self.name, self.data, self.nd, self.info = name, data, nd, info


# ---- the hash-free checker --------------------------------------------------------------------------------------------------------------
def valid_dedup(stream, d):
    """Problems of a stream as a de-duplicated serialization of `d`, for ANY table policy (an empty list: none): every string
    entry's (offset, length) spells its string inside the column; the column is the concatenation, in tape order, of a subset of
    the non-empty string entries; the subset holds the first occurrence of every distinct string; an entry outside it points at
    its string's first occurrence.  Tags and all other values are the model's."""
    u = unframe(stream)
    scol, tags, vals = d.columns(False)
    col = u["strings"]
    if u["tape_len"] != d.n or u["tags"] != tags:
        return ["tape length or tag column"]
    got = np.frombuffer(u["values"], dtype=np.uint64).tolist()
    if len(got) != len(vals):
        return ["value column length"]
    is_off = [False] * len(vals)
    for k, _ in d.strs:
        is_off[d.vstart[k] // 8] = True
    if any(a != b for a, b, o in zip(got, vals, is_off) if not o):
        return ["a value that is no string offset"]
    bad, cur, first, subset, off = [], 0, {}, set(), {}
    for k, s in d.strs:
        o = got[d.vstart[k] // 8]
        off[k] = o
        if col[o:o + len(s)] != s:
            bad.append(("entry %d does not spell its string" % k, o))
        first.setdefault(s, k)
        if s and o == cur:
            subset.add(k)
            cur += len(s)
    if cur != len(col):
        bad.append(("the column is not the kept entries in tape order", cur, len(col)))
    for k, s in d.strs:
        if not s:
            continue
        f = first[s]
        if f not in subset:
            bad.append("first occurrence %d of a string is not in the column" % f)
        elif k not in subset and off[k] != off[f]:
            bad.append("entry %d does not point at the first occurrence %d" % (k, f))
    return bad


def owner(d, column, byte, dedup=False):
    """the entry that owns `byte` of a column ('tags', 'values', 'strings') -> (tile, thread, tape word, entry label, entry index)"""
    scol, tags, vals = d.columns(dedup)
    if column == "tags":
        k = min(byte, len(d.kinds) - 1)
    elif column == "values":
        k = int(np.searchsorted(np.array(d.vstart), byte, side="right")) - 1
        while d.kinds[k] in ("]", "}", "true", "false", "null"):  # (entries without a value share their successor's offset)
            k -= 1
    else:
        starts, ks = [], []
        if dedup:
            _, off = d.string_column(*d.plan)
            for k, s in d.strs:
                if k in d.plan[0]:
                    starts.append(off[k])
                    ks.append(k)
        else:
            ks = [k for k, _ in d.strs]
            starts = [d.soffs[k] for k in ks]
        if not ks:
            return None
        k = ks[max(0, int(np.searchsorted(np.array(starts), byte, side="right")) - 1)]
    w = int(d.words[k])
    return w // TILE, w % TILE // ITEMS, w, d.label(k), k


def describe(d, got, dedup):
    """the first difference between a stream and the model's, for an assertion message"""
    want, got = d.stream(dedup), bytes(got)
    if got == want:
        return None
    k = next(i for i in range(min(len(got), len(want)) + 1) if got[i:i + 1] != want[i:i + 1])
    u = unframe(want)
    where = ("header", k, None)
    for name in ("strings", "tags", "values"):
        if u["at"][name] <= k < u["at"][name] + len(u[name]):
            where = (name, k - u["at"][name], owner(d, name, k - u["at"][name], dedup))
    return (d.name, "dedup" if dedup else "plain", "lengths", len(got), len(want), "first difference at stream byte", k, "column", where[0],
            "byte", where[1], "got", got[max(0, k - 8):k + 8].hex(), "want", want[max(0, k - 8):k + 8].hex(),
            "owner (tile, thread, tape word, entry, index)", where[2])


# ---- placing an entry kind --------------------------------------------------------------------------------------------------------------
KINDS = ("key", "str", "empty", "int", "uint", "float", "e", "{", "[", "}", "]", "true", "false", "null", "R", "r")
# label -> (entries, number of one-word, one-tag entries in front of the entry meant)
SEQ = {"key": ([("{",), ("key", b"k\"y"), ("int", 8), ("}",)], 1), "str": ([("str", b"ed\tge")], 0), "empty": ([("str", b"")], 0),
       "int": ([("int", -12345)], 0), "uint": ([("uint", (1 << 63) + 5)], 0), "float": ([("float", -2.5e-7)], 0), "e": ([("e", 3)], 0),
       "{": ([("{",), ("}",)], 0), "[": ([("[",), ("]",)], 0), "}": ([("{",), ("}",)], 1), "]": ([("[",), ("]",)], 1),
       "true": ([("true",)], 0), "false": ([("false",)], 0), "null": ([("null",)], 0)}


def place(b, label, target, by="word"):
    """entries that put the tag of an entry of kind `label` on tape word (or tag index) `target`"""
    fill = b.fill if by == "word" else b.fill_tags
    if label in ("R", "r"):
        fill(target - (1 if label == "R" else 2))
        b.extend([("]",), ("rec",), ("[",)])
        return
    ents, front = SEQ[label]
    fill(target - front)
    for e in ents:
        b.put(e)


# ---- a. entries on thread and tile edges -----------------------------------------------------------------------------------------------
A_EDGES = ("item7", "wave0", "wave1", "wave2", "t2047", "t2048", "t2049")
A_LENGTHS = tuple(TILE * k + r for k in (1, 2) for r in (-1, 0, 1, 2))


def edge_classes(w):
    """the edges of the serializer's walk a tag on tape word w lies on"""
    out = set()
    r = w % TILE
    if r % ITEMS == ITEMS - 1 and r != TILE - 1:
        out.add("item7")  # ... its second word is the thread's look-ahead
    for i in range(3):
        if r == (i + 1) * WAVE_WORDS - 1:
            out.add("wave%d" % i)
    if r == TILE - 1:
        out.add("t2047")
    if r == 0 and w:
        out.add("t2048")
    if r == 1 and w > TILE:
        out.add("t2049")
    return out


def a_item7_doc():
    b = Builder(True)
    b.add("[")
    i = 1
    for label in KINDS:
        while (24 * i + 7) % TILE in (TILE - 1,) or (24 * i + 7) % WAVE_WORDS == WAVE_WORDS - 1:
            i += 1
        place(b, label, 24 * i + 7)
        i += 1
    b.fill(b.word + 3)
    b.add("]")
    return b.done("a item 7 of a thread", {"family": "a"})


def a_tile_doc():
    """kind k in tiles 3k .. 3k + 3: the last word of waves 0, 1, 2 and of the tile, the first word of tile 3k + 2, the second of 3k + 3"""
    b = Builder(True)
    b.add("[")
    for k, label in enumerate(KINDS):
        t0 = 3 * k * TILE
        for target in (t0 + WAVE_WORDS - 1, t0 + 2 * WAVE_WORDS - 1, t0 + 3 * WAVE_WORDS - 1, t0 + TILE - 1, t0 + 2 * TILE, t0 + 3 * TILE + 1):
            place(b, label, target)
    b.fill(b.word + 3)
    b.add("]")
    return b.done("a wave and tile edges", {"family": "a"})


def a_length_docs():
    """tapes of 2048 k + {-1, 0, 1, 2} words: the closing root on words 2047, 2048 and 2049 of a tile, the last thread with 7, 8, 1
    and 2 words; a string is the last entry"""
    for n in A_LENGTHS:
        b = Builder()
        b.add("[")
        b.fill(n - 4)
        b.extend([("str", b"la\\st"), ("]",)])
        yield b.done("a n=%d" % n, {"family": "a", "n": n})


def a_observed(docs):
    return {(d.label(k), c) for d in docs for k, w in enumerate(d.words.tolist()) for c in edge_classes(w)}


def family_a():
    yield a_item7_doc()
    yield a_tile_doc()
    yield from a_length_docs()


# ---- b. the anchor search and the retry ---------------------------------------------------------------------------------------------------
B_DISTANCES = (62, 63, 64, 65, 66, 67)
B_POSITIONS = ("first", "middle", "last")
B_TILES = 4
B_REPEATED = (b"alpha", b"a repeated string of 33 bytes ...", b"x", b"")


def b_doc(dist, pos):
    """the last anchor `dist` words in front of the start of tile 1 (the first that can miss it), 2 (a middle one) or 3 (the last):
    behind it only raw words whose top byte is one of \" l u d.  The anchor is a null or the raw word of a uint in turn; the run
    holds floats and integers.  Repeated strings lie in front of the tile, inside it and behind it."""
    edge_tile = B_POSITIONS.index(pos) + 1
    edge = edge_tile * TILE
    run = dist // 2
    b = Builder()
    b.add("[")
    for s in B_REPEATED:
        b.add("str", s)
    if edge_tile > 1:
        b.fill((edge_tile - 1) * TILE + 10)
        b.extend([("{",), ("key", B_REPEATED[0]), ("str", B_REPEATED[1]), ("}",)])
    if (dist + edge_tile) % 2:
        b.fill(edge - dist - 1)
        b.add("uint", (1 << 63) + dist)
    else:
        b.fill(edge - dist)
        b.add("null")
    assert b.word == edge - dist + 1
    for i in range(run + 2):  # (the run goes on behind the edge)
        b.add(*M.number_with_top(M.TWO_WORD_TOPS[i % 4], i, (i + dist) % 3 != 0))
    for s in B_REPEATED + (b"only in tile %d" % edge_tile,):
        b.add("str", s)
    b.extend([("{",), ("key", B_REPEATED[0]), ("[",), ("int", 1), ("]",), ("key", B_REPEATED[2]), ("str", B_REPEATED[1]), ("}",)])
    b.fill((B_TILES - 1) * TILE + 200)
    for s in B_REPEATED:
        b.add("str", s)
    b.add("]")
    return b.done("b anchor %d in front of tile %d (%s)" % (dist, edge_tile, pos),
                  {"family": "b", "dist": dist, "pos": pos, "edge": edge, "retry": dist > REACH})


def b_observed(d):
    """(distance of the closest anchor in front of a tile, the tile's first word is raw, position) of every tile but the first"""
    two = np.isin(d.tape >> np.uint64(56), np.array(M.TWO_WORD_TOPS, dtype=np.uint64))
    tagw = set(d.words.tolist())
    out = set()
    for t in range(1, d.tiles):
        p = t * TILE - 1
        while two[p]:
            p -= 1
        out.add((t * TILE - p, t * TILE not in tagw, "first" if t == 1 else "last" if t == d.tiles - 1 else "middle"))
    return out


def family_b():
    for dist in B_DISTANCES:
        for pos in B_POSITIONS:
            yield b_doc(dist, pos)


# ---- c. de-duplication seams ----------------------------------------------------------------------------------------------------------------
C_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65)
C_PLACEMENTS = {"one thread": (16, 18), "neighbouring threads": (30, 32), "different waves": (100, 600),
                "neighbouring tiles": (2000, TILE + 10), "3 tiles apart": (TILE + 52, 4 * TILE + 52)}
# (length, the one byte that differs): only bytes that two or more steps of the hash follow.  Strings that differ in one byte of
# the last word or of the tail never share a slot (the last products differ in too few bits), so ser_equal never sees them.
C_DIFFER = ((16, 0), (17, 0), (64, 0), (24, 8), (65, 8), (32, 16), (65, 16))
# lengths of pairs that are equal up to their last 8 bytes (ser_equal fails in its last word or in its byte tail)
C_TAILS = (7, 8, 9, 15, 16, 17, 63, 64, 65)
_ALPHA = bytes(c for c in range(0x20, 0x7F) if c not in (0x22, 0x5C))


def _letters(rnd, n):
    return bytes(rnd.choice(_ALPHA) for _ in range(n))


def placement(w1, w2):
    if w1 // TILE != w2 // TILE:
        return "neighbouring tiles" if w2 // TILE - w1 // TILE == 1 else "%d tiles apart" % (w2 // TILE - w1 // TILE)
    if w1 // ITEMS == w2 // ITEMS:
        return "one thread"
    if w1 // WAVE_WORDS != w2 // WAVE_WORDS:
        return "different waves"
    return "neighbouring threads" if w2 // ITEMS - w1 // ITEMS == 1 else "one wave"


@functools.lru_cache(maxsize=None)
def collisions():
    """pairs of different strings in one slot of the table, found with the mirrored hash -> dict:
    'equal': 8-byte strings; 'unequal': strings of different lengths; ('differ', n, p): strings of n bytes that differ in byte p
    only; 'prefix': one a proper prefix of the other"""
    rnd = random.Random(20261019)
    out, seen = {}, {}
    for _ in range(20000):
        s = _letters(rnd, 8)
        o = seen.setdefault(ser_hash(s), s)
        if o != s:
            out.setdefault("equal", []).append((o, s))
    seen = {}
    while "unequal" not in out:
        s = _letters(rnd, rnd.randrange(3, 14))
        o = seen.setdefault(ser_hash(s), s)
        if len(o) != len(s):
            out["unequal"] = [(o, s)]
    for n, p in C_DIFFER:
        for _ in range(20000):
            if ("differ", n, p) in out:
                break
            base, seen = bytearray(_letters(rnd, n)), {}
            for c in _ALPHA:
                base[p] = c
                o = seen.setdefault(ser_hash(base), bytes(base))
                if o != base:
                    out["differ", n, p] = [(o, bytes(base))]
                    break
    for n in C_TAILS:
        base, seen = _letters(rnd, n), {}
        for _ in range(200000):
            s = base[:max(0, n - 8)] + _letters(rnd, min(n, 8))
            o = seen.setdefault(ser_hash(s), s)
            if o != s:
                out["tail", n] = [(o, s)]
                break
    while "prefix" not in out:
        base, seen = _letters(rnd, 200), {}
        for n in range(1, 201):
            o = seen.setdefault(ser_hash(base[:n]), base[:n])
            if len(o) != n:
                out["prefix"] = [(o, base[:n])]
                break
    return out


def c_placement_doc():
    """a string and its repeat in one thread, neighbouring threads, different waves, neighbouring tiles and 3 tiles apart; as a key
    after a value and as a value after a key; spelled with an escape after it was seen raw"""
    items = []
    for name, (w1, w2) in C_PLACEMENTS.items():
        items += [(w1, ("str", b"placed " + name.encode())), (w2, ("str", b"placed " + name.encode()))]
    b = Builder()
    b.add("[")
    for w, e in sorted(items):
        b.fill(w)
        b.add(*e)
    for e in (("str", b"value first"), ("{",), ("key", b"value first"), ("int", 1), ("key", b"key first"), ("int", 2), ("}",), ("str", b"key first"),
              ("str", b"Ab"), ("spelled", "str", b"Ab", b'"\\u0041b"'), ("{",), ("spelled", "key", b"Ab", b'"A\\u0062"'), ("null",), ("}",)):
        b.put(e)
    b.add("]")
    return b.done("c placements", {"family": "c"})


def c_order_docs():
    col = collisions()
    for name, pairs in (("equal", col["equal"][:3]), ("unequal", col["unequal"])):
        for j, (x, y) in enumerate(pairs):
            for order, keeps in (("ABBAB", {"A": 1, "B": 3}), ("BAAB", {"B": 1, "A": 2})):
                ents = [("[",)] + [("str", x if c == "A" else y) for c in order] + [("]",)]
                b = Builder()
                b.extend(ents)
                yield b.done("c collision %s %d %s" % (name, j, order), {"family": "c", "order": order, "lengths": name, "keeps": keeps,
                                                                      "A": x, "B": y})


def c_length_doc():
    """every length twice; pairs in one slot that differ in one byte (the last, byte 8, byte 16, byte 0) or in length only, as
    X Y X Y: X is the slot's first and kept once, Y meets X's bytes every time and is kept twice"""
    b = Builder()
    b.add("[")
    for n in C_LENGTHS:
        s = (b"%d:" % n + b"abcdefghijklmnopqrstuvwxyz" * 3)[:n]
        b.extend([("str", s), ("int", n), ("str", s)])
    col = collisions()
    lay = []
    for key in [("differ", n, p) for n, p in C_DIFFER] + [("tail", n) for n in C_TAILS] + ["prefix"]:
        x, y = col[key][0]
        b.extend([("str", x), ("str", y), ("{",), ("key", x), ("str", y), ("}",)])
        lay.append((key, x, y))
    b.add("]")
    return b.done("c lengths and near-equal pairs", {"family": "c", "lay": lay})


def c_align_doc():
    """first occurrence at Strings.B offset a mod 8, repeat at b mod 8, all 64 (a, b); the lengths in rotation"""
    b = Builder()
    b.add("[")
    so, lens, lay = 0, [n for n in C_LENGTHS if n], []

    def pad(to, tag):
        nonlocal so
        n = (to - so) % 8
        if n:
            b.add("str", (tag + b"#######")[:n])
            so += n
    for a in range(8):
        for r in range(8):
            n = lens[(a * 8 + r) % len(lens)]
            s = (_ALPHA[30 + a * 8 + r:31 + a * 8 + r] + b"%d%d" % (a, r) + b"ABCDEFGHIJKLMNOPQRSTUVWXYZ" * 3)[:n]  # (distinct in its first byte)
            pad(a, b"%d" % r)
            b.add("str", s)
            so += n
            pad(r, b"%d" % a)
            b.add("str", s)
            so += n
            lay.append((a, r, n))
    b.add("]")
    return b.done("c alignments", {"family": "c", "lay": lay})


def c_align_observed(d):
    """(offset mod 8 of a string's first occurrence, of a repeat, length)"""
    first, out = {}, set()
    for k, s in d.strs:
        if s in first:
            out.add((first[s] % 8, d.soffs[k] % 8, len(s)))
        else:
            first[s] = d.soffs[k]
    return out


def c_heavy_doc():
    """tile 1 keeps more than 64 KiB, tile 2 nothing (repeats and numbers only), tile 3 some"""
    b = Builder()
    b.add("[")
    b.fill(TILE)
    big = [(b"%02d" % i) * 1100 for i in range(32)]
    for s in big:
        b.add("str", s)
    b.fill(2 * TILE)
    for s in big[:5]:
        b.add("str", s)
    b.fill(3 * TILE)
    b.extend([("str", big[7]), ("str", b"kept in tile 3"), ("str", b"zz" * 1100), ("]",)])
    return b.done("c heavy tile", {"family": "c"})


def kept_bytes_per_tile(d):
    out = [0] * d.tiles
    for k, s in d.strs:
        if k in d.plan[0]:
            out[int(d.words[k]) // TILE] += len(s)
    return out


def c_degenerate_docs():
    b = Builder()
    b.extend([("[",), ("int", 1), ("true",), ("{",), ("}",), ("]",)])
    yield b.done("c no string", {"family": "c"})
    b = Builder()
    b.extend([("{",), ("key", b""), ("[",), ("str", b""), ("str", b""), ("]",), ("}",)])
    yield b.done("c empty strings only", {"family": "c"})
    b = Builder()
    b.add("[")
    for _ in range(3000):
        b.add("str", b"one distinct string")
    b.add("]")
    yield b.done("c one string 3000 times", {"family": "c"})


def family_c():
    yield c_placement_doc()
    yield from c_order_docs()
    yield c_length_doc()
    yield c_align_doc()
    yield c_heavy_doc()
    yield from c_degenerate_docs()


# ---- d. extremes of the packed counts -------------------------------------------------------------------------------------------------------
D_FORMS = ("atoms", "openers", "strings", "e floats")


def d_doc(form):
    """tile 1 holds exactly 2048 one-word entries without a value, 1024 openers with their closers (the parser's depth is limited:
    [[],[],...]), 1024 strings, or 1024 flagged floats"""
    b = Builder()
    b.add("[")
    b.fill(TILE)
    for i in range(TILE // 2):
        if form == "atoms":
            b.extend([("null",), ("true",)])
        elif form == "openers":
            b.extend([("[",), ("]",)])
        elif form == "strings":
            b.add("str", b"s%d" % (i % 300))
        else:
            b.add_e(i)
    assert b.word == 2 * TILE
    b.extend([("int", 5), ("]",)])
    return b.done("d tile of " + form, {"family": "d", "form": form})


def d_observed(d, tile=1):
    """(entries, value bytes) of a tile, by label"""
    c = {}
    for k, w in enumerate(d.words.tolist()):
        if w // TILE == tile:
            c[d.label(k)] = c.get(d.label(k), 0) + 1
    return c


def family_d():
    for form in D_FORMS:
        yield d_doc(form)


# ---- e. frame widths --------------------------------------------------------------------------------------------------------------------
E_STEPS = (126, 127, 128, 16382, 16383, 16384)
E_VALUE_STEPS = (120, 128, 136, 16376, 16384, 16392)
E_QUANTITIES = ("tape", "strings", "strings dedup", "tags", "values", "rest")


def e_docs():
    def nulls(k, name, extra=()):
        b = Builder()
        b.add("[")
        for e in extra:
            b.add(*e)
        for _ in range(k):
            b.add("null")
        b.add("]")
        return b.done(name, {"family": "e"})
    for n in E_STEPS:
        yield nulls(n - 4, "e tape and tags %d" % n)  # r [ null * k ] r: k + 4 words, k + 4 tags
        yield nulls(0, "e string column %d" % n, [("str", b"s" * n)])
        yield nulls(0, "e string column %d after de-duplication" % n, [("str", b"t" * n), ("str", b"t" * n)])
    for v in E_VALUE_STEPS:
        b = Builder()
        b.add("[")
        for _ in range((v - 24) // 8):  # (the two roots and the array: 8 bytes each)
            b.add("int", 7)
        b.add("]")
        yield b.done("e value column %d" % v, {"family": "e"})
    for r in E_STEPS:
        hit = None
        for k in range(4):
            for m in range(max(1, r - 80), r):
                if rest_len(6 + k, m, 5 + k, 40) == r:
                    hit = (k, m)
        assert hit, r
        yield nulls(hit[0], "e rest %d" % r, [("str", b"r" * hit[1])])


def e_observed(d):
    out = set()
    for dedup in (False, True):
        u = unframe(d.stream(dedup))
        out |= {("tape", u["tape_len"]), ("strings dedup" if dedup else "strings", len(u["strings"])), ("tags", len(u["tags"])),
                ("values", len(u["values"])), ("rest", u["rest"])}
    return out


def family_e():
    yield from e_docs()


# ---- f. scan cuts of the serializer, g. the tag column on Deserialize's cuts ---------------------------------------------------------------
F_TILES = (1, 2, 15, 16, 17, 1023, 1024, 1025)
G_TILES = (1, 2, 16, 17, 1024, 1025)
G_TAGS = tuple(DS_TILE * k + r for k in (1, 2) for r in (-1, 0, 1))
G_EDGES = ("item15", "t4095", "t4096", "t4097")


def f_doc(tiles):
    """`tiles` serializer tiles of integers: the last tile holds about a third of its words"""
    n = (tiles - 1) * TILE + 700
    if tiles <= 2:
        b = Builder()
        b.add("[")
        b.fill(n - 2)
        b.add("]")
        return b.done("f %d tiles" % tiles, {"family": "f", "tiles": tiles, "n": n})
    k = (n - 4) // 2
    return BigDoc("f %d tiles" % tiles, b"[" + b"1," * (k - 1) + b"1]", {"family": "f", "tiles": tiles, "n": n})


def family_f():
    for t in F_TILES:
        yield f_doc(t)


def tag_edge_classes(i):
    out = set()
    r = i % DS_TILE
    if r % DS_ITEMS == DS_ITEMS - 1 and r != DS_TILE - 1:
        out.add("item15")
    if r == DS_TILE - 1:
        out.add("t4095")
    if r == 0 and i:
        out.add("t4096")
    if r == 1 and i > DS_TILE:
        out.add("t4097")
    return out


def g_kind_doc(edge):
    """every kind on tag 15 of a thread, or on tag 4095, 4096 or 4097 of a tile (one tile edge per kind)"""
    b = Builder(True)
    b.add("[")
    for j, label in enumerate(KINDS):
        target = 48 * (j + 1) + 15 if edge == "item15" else DS_TILE * (j + 1) + {"t4095": -1, "t4096": 0, "t4097": 1}[edge]
        place(b, label, target, by="tag")
    b.fill_tags(b.ntags + 3)
    b.add("]")
    return b.done("g kinds on %s" % edge, {"family": "g", "edge": edge})


def g_count_doc(tags):
    b = Builder()
    b.add("[")
    b.fill_tags(tags - 2)
    b.add("]")
    return b.done("g %d tags" % tags, {"family": "g", "tags": tags})


def g_bracket_doc():
    """an opener whose closer lies in the next tag tile, one whose closer lies 3 tag tiles on, and NDJSON records whose roots
    straddle tag tiles"""
    b = Builder(True)
    b.add("[")
    b.fill_tags(100)
    b.extend([("{",), ("key", b"far"), ("[",)])   # tags 100 and 102: closed 3 tag tiles on
    b.fill_tags(DS_TILE - 96)
    b.add("[")                                       # tag 4000: closed on tag 4200, in the next tag tile
    b.fill_tags(DS_TILE + 104)
    b.add("]")
    b.fill_tags(3 * DS_TILE + 100)
    b.extend([("]",), ("}",), ("]",), ("rec",), ("[",)])
    b.fill_tags(4 * DS_TILE - 2)
    b.extend([("]",), ("rec",), ("{",)])             # a record's closing root on tag 16383, the next opening root on 16384
    b.extend([("key", b"k"), ("[",)])
    b.fill_tags(5 * DS_TILE + 7)
    b.extend([("]",), ("}",)])
    return b.done("g brackets and roots across tag tiles", {"family": "g", "brackets": True})


def bracket_spans(d):
    """(tag tile of the opener, tag tile of its closer) of every bracket pair and root pair"""
    out, stack = set(), []
    for i, kd in enumerate(d.kinds):
        if kd in ("[", "{", "r"):
            stack.append(i)
        elif kd in ("]", "}", "R"):
            out.add((kd, stack.pop() // DS_TILE, i // DS_TILE))
    return out


def g_tiles_doc(tiles):
    n = (tiles - 1) * DS_TILE + 1500
    if tiles <= 2:
        return g_count_doc(n)
    return BigDoc("g %d tag tiles" % tiles, b"[" + b"null," * (n - 5) + b"null]", {"family": "g", "tag_tiles": tiles, "tags": n})


def family_g():
    for edge in G_EDGES:
        yield g_kind_doc(edge)
    for n in G_TAGS:
        yield g_count_doc(n)
    yield g_bracket_doc()
    for t in G_TILES:
        yield g_tiles_doc(t)


# ---- h. corrupt streams ---------------------------------------------------------------------------------------------------------------------
def h_base():
    """a well-formed stream of two tag tiles: an opener on tag 4000 whose closer is tag 4200, across the cut, an opener and its
    closer in tile 1 (tags 4300, 4310), a string, numbers"""
    b = Builder()
    b.add("[")
    b.extend([("str", b"h"), ("int", -1), ("float", 0.5)])
    b.fill_tags(DS_TILE - 96)
    b.add("[")
    b.fill_tags(DS_TILE + 104)
    b.add("]")
    b.fill_tags(DS_TILE + 204)
    b.add("[")
    b.fill_tags(DS_TILE + 214)
    b.add("]")
    b.fill_tags(DS_TILE + 400)
    b.add("]")
    return b.done("h base", {"family": "h"})


def h_streams():
    """-> (the base document, its stream, [(name, mutated stream)])"""
    d = h_base()
    scol, tags, vals = d.columns(False)
    n, nt = d.n, len(tags)
    vb = np.array(vals, dtype=np.uint64).tobytes()
    good = frame(n, scol, tags, vb)
    assert good == d.stream(False) and d.tag_tiles == 2
    assert [d.kinds[i] for i in (DS_TILE - 96, DS_TILE + 104, DS_TILE + 204, DS_TILE + 214)] == ["[", "]", "[", "]"]
    out = []

    def with_tag(i, c):
        t = bytearray(tags)
        t[i] = c
        return frame(n, scol, bytes(t), vb)

    def with_value(k, v):
        x = list(vals)
        x[d.vstart[k] // 8] = v & U64
        return frame(n, scol, tags, np.array(x, dtype=np.uint64).tobytes())
    assert tags[DS_ITEMS - 1] == tags[DS_TILE - 1] == ord("n") and tags[nt - 1] == ord("r")
    for where, i in (("thread", DS_ITEMS - 1), ("tile", DS_TILE - 1), ("column", nt - 1)):
        out.append(("unknown tag on the last tag of a %s" % where, with_tag(i, ord("X"))))
        out.append(("TagNop on the last tag of a %s" % where, with_tag(i, ord("N"))))
    out.append(("value column one entry short", frame(n, scol, tags, vb[:-8])))
    out.append(("value column one entry long", frame(n, scol, tags, vb + bytes(8))))
    out.append(("tape_len one less", frame(n - 1, scol, tags, vb)))
    out.append(("tape_len one more", frame(n + 1, scol, tags, vb)))
    a, a_close, c, c_close = DS_TILE - 96, DS_TILE + 104, DS_TILE + 204, DS_TILE + 214
    wa = int(d.words[a])
    out.append(("opener whose distance ends at tape_len", with_value(a, n - wa)))
    out.append(("opener whose distance ends one past tape_len", with_value(a, n + 1 - wa)))
    out.append(("opener of tile 0 claims the closing slot of an opener of tile 1", with_value(a, int(d.words[c_close]) + 1 - wa)))
    out.append(("opener of tile 1 claims the closing slot of an opener of tile 0", with_value(c, int(d.words[a_close]) + 1 - int(d.words[c]))))
    out.append(("closing tag of the wrong kind across the tile cut", with_tag(a_close, ord("}"))))
    u = unframe(good)
    for o in u["header"][1:]:
        out.append(("stream cut in front of header byte %d" % o, good[:o]))
    out.append(("stream cut in front of its last byte", good[:-1]))
    for i, col in enumerate(("string", "tag", "value")):
        out.append(("%s block size is its size" % col, frame(n, scol, tags, vb, bsize_delta=(i, -1))))
        out.append(("%s block size is its size + 2" % col, frame(n, scol, tags, vb, bsize_delta=(i, 1))))
        out.append(("%s block type 1" % col, frame(n, scol, tags, vb, btype=(i, 1))))
    out.append(("tag block sizes that wrap 64 bits", frame(n, scol, tags, vb, sizes=(1, U64 - 1, U64))))
    out.append(("version 4", frame(n, scol, tags, vb, version=4)))
    out.append(("rest one more than the stream holds", frame(n, scol, tags, vb, rest_delta=1)))
    return d, good, out


FAMILIES = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e, "f": family_f, "g": family_g}


@functools.lru_cache(maxsize=None)
def family(name):
    return tuple(FAMILIES[name]())
