"""Where stage 2's bracket matcher (csrc/stage2.hip) cuts the brackets of a message, a plain mirror that says which part of
the matcher answers every bracket, and documents that put a question on each of those cuts.  No GPU import.

The kernels.  k_s2_emit_planes lists the brackets of its tile of S2_TILE = 4096 tokens (a token is one structural index of
stage 1; in NDJSON the record separators are tokens too) and writes the compact bracket view: bracket c of the message has
br_depth[c] = the nesting depth BEHIND it (an open bracket counts itself, a close bracket does not).  Every bracket asks one
previous-smaller-value question q = depth in front of it - 1 (a close: dep, an open: dep - 2): the answer a is the last
bracket in front with depth <= q, and a + 1 is the container of the gap in front of the bracket -- the partner of a close,
the parent of an open; no answer means bracket 0.  q < 0 is the root context and asks nothing.

Liveness (stage2.hip, the `root` / `res >= 0` / `done` lines of the tile matcher): the tile answers a question only with
a bracket of its own list (res is an index inside the tile and res + 1 <= the asking bracket), so a bracket is DONE iff
q < 0 or a lies in the bracket's own tile; it is live -- left to k_br_match -- iff q >= 0 and a is in a tile in front or
does not exist.  A container that starts as the first bracket of a tile is therefore live at its close although both ends
lie in the tile, and so is every direct child of it.

k_br_match takes the live brackets of a group of 64 (compact index >> 6) and finds a
    own_group        among the lanes below it (ballot on depth == q);
    none_g0          nowhere: group 0 has no group in front (res stays -1);
    group_in_front   in the 64 depths of group g - 1;
    none_idx0        nowhere: wave_psv_tree(L = 1, idx = g - 1) with idx == 0 (g == 1);
    tree(L)          by wave_psv_tree: at level L the window [hb, idx), hb = ((idx - 1) >> 6) << 6, is the first to hold an
                     entry <= q; the climb goes on with idx = hb >> 6 at level L + 1;
    none_hb0         nowhere: a window that starts at entry 0 holds nothing;
    none_top         nowhere: the top level is exhausted with hb != 0.  Unreachable: the top level of make_tree has at most
                     64 entries unless MAXLEV = 7 levels cap it, and n_br is a 32-bit count (< 64^6).

The mirror is an instrument for the CPU tests (does the set of documents reach every part at every edge?); the verdict of
the GPU tests is the oracle's tape alone."""
import collections

import numpy as np

S2_TILE = 4096
MAXLEV = 7  # sj_stage2.h MinTree::MAXLEV
BIG = 0x7FFFFFFF

_OPEN_ARR, _OPEN_OBJ, _CLOSE_ARR, _CLOSE_OBJ = 0x5B, 0x7B, 0x5D, 0x7D


class View:
    """the brackets of a document in order: tok (token index), pos (byte offset), ch (the byte), is_close, depth (as
    br_depth), off (tape offset of the bracket's word, as br_off), tile, q"""

    def __init__(self, doc, positions):
        a = np.frombuffer(bytes(doc) if not isinstance(doc, np.ndarray) else doc, dtype=np.uint8)
        positions = np.asarray(positions, dtype=np.int64)
        ch = a[positions]
        opens = (ch == _OPEN_ARR) | (ch == _OPEN_OBJ)
        closes = (ch == _CLOSE_ARR) | (ch == _CLOSE_OBJ)
        self.n_tokens = len(positions)
        self.tok = np.flatnonzero(opens | closes)
        self.pos = positions[self.tok]
        self.ch = ch[self.tok]
        self.is_close = closes[self.tok]
        self.depth = np.cumsum(np.where(self.is_close, -1, 1)).astype(np.int64)
        self.tile = self.tok // S2_TILE
        self.q = np.where(self.is_close, self.depth, self.depth - 2)
        self.n = len(self.tok)
        # tape words: an atom and a bracket take one, a string and a number two; a container at depth 0 has a root word
        # in front of its open and one behind its close (the documents of this module hold no scalar records)
        words = np.zeros(len(ch), dtype=np.int64)
        words[opens | closes | (ch == ord("t")) | (ch == ord("f")) | (ch == ord("n"))] = 1
        words[(ch == 0x22) | (ch == ord("-")) | ((ch >= ord("0")) & (ch <= ord("9")))] = 2
        dtok = np.zeros(len(ch), dtype=np.int64)
        dtok[self.tok] = np.where(self.is_close, -1, 1)
        dafter = np.cumsum(dtok)
        words[opens & (dafter == 1)] += 1   # the root word in front counts with the open
        root_close = closes & (dafter == 0)
        before = np.cumsum(words) - words + np.cumsum(root_close) - root_close
        self.off = before[self.tok] + (opens & (dafter == 1))[self.tok]

    def answers(self):
        """a for every bracket (-1: none; meaningless where q < 0).  Depths of neighbours differ by one, so the last
        bracket in front with depth <= q is the last one with depth == q: one sort by (depth, index)"""
        n = self.n
        order = np.argsort(self.depth, kind="stable")
        keys = self.depth[order] * (n + 1) + order
        at = np.searchsorted(keys, self.q * (n + 1) + np.arange(n)) - 1
        cand = order[np.maximum(at, 0)]
        ok = (at >= 0) & (self.depth[cand] == self.q) & (cand < np.arange(n))
        return np.where(ok, cand, -1)

    def answer_by_scan(self, c):
        """the same by a plain scan over everything in front of bracket c"""
        hit = np.flatnonzero(self.depth[:c] <= self.q[c])
        return int(hit[-1]) if len(hit) else -1

    def live(self, a=None):
        a = self.answers() if a is None else a
        return (self.q >= 0) & ((a < 0) | (self.tile[np.maximum(a, 0)] != self.tile))

    def levels(self):
        """make_tree + the minima tree12_body / k_min_upper leave: [depth, level 1, ...]"""
        lev = [self.depth]
        sz = self.n
        while sz > 64 and len(lev) < MAXLEV:
            cur = lev[-1]
            pad = (-len(cur)) % 64
            cur = np.concatenate([cur, np.full(pad, BIG, dtype=np.int64)]) if pad else cur
            lev.append(cur.reshape(-1, 64).min(axis=1))
            sz = (sz + 63) // 64
        return lev


CLASSES = ["own_group", "none_g0", "group_in_front", "none_idx0", "none_hb0", "none_top"] + ["tree(%d)" % L for L in range(1, MAXLEV)]
Walk = collections.namedtuple("Walk", "cls a level hit_first hit_last idx_mult64")


def walk(view, lev, c):
    """k_br_match + wave_psv_tree for bracket c, window by window on the level arrays, as the kernel's loops go"""
    q = int(view.q[c])
    g = c >> 6
    hit = np.flatnonzero(lev[0][g * 64:c] == q)
    if len(hit):
        return Walk("own_group", g * 64 + int(hit[-1]), 0, False, False, False)
    if g == 0:
        return Walk("none_g0", -1, 0, False, False, False)
    hit = np.flatnonzero(lev[0][(g - 1) * 64:g * 64] <= q)
    if len(hit):
        return Walk("group_in_front", (g - 1) * 64 + int(hit[-1]), 0, int(hit[-1]) == 0, int(hit[-1]) == 63, False)
    nlev = len(lev)
    L, idx, mult = 1, g - 1, False
    while True:
        if idx == 0:
            return Walk("none_idx0", -1, L, False, False, mult)
        mult |= idx % 64 == 0
        hb = ((idx - 1) >> 6) << 6
        hit = np.flatnonzero(lev[L][hb:idx] <= q)
        if len(hit):
            h = hb + int(hit[-1])
            break
        if hb == 0:
            return Walk("none_hb0", -1, L, False, False, mult)
        if L + 1 >= nlev:
            return Walk("none_top", -1, L, False, False, mult)
        idx = hb >> 6
        L += 1
    level, first, last = L, h == hb, h == idx - 1
    while L > 0:
        L -= 1
        hit = np.flatnonzero(lev[L][h << 6:(h << 6) + 64] <= q)
        h = (h << 6) + int(hit[-1])
    return Walk("tree(%d)" % level, h, level, first, last, mult)


def classify(view, a=None):
    """every live bracket at once, from its answer: -> (c, a, cls, level, hit_first, hit_last, idx_mult64) arrays; cls
    indexes CLASSES.  tests/test_s2_brackets.py holds it against walk()."""
    a_all = view.answers() if a is None else a
    c = np.flatnonzero(view.live(a_all))
    a = a_all[c]
    n = len(c)
    nlev = 1 + sum(1 for _ in _level_sizes(view.n))
    g = c >> 6
    cls = np.full(n, -1, dtype=np.int8)  # index into CLASSES
    level = np.zeros(n, dtype=np.int64)
    first = np.zeros(n, dtype=bool)
    last = np.zeros(n, dtype=bool)
    mult = np.zeros(n, dtype=bool)
    own = (a >= 0) & ((a >> 6) == g)
    cls[own] = CLASSES.index("own_group")
    g0 = ~own & (g == 0)
    cls[g0] = CLASSES.index("none_g0")
    front = ~own & ~g0 & (a >= 0) & ((a >> 6) == g - 1)
    cls[front] = CLASSES.index("group_in_front")
    first[front] = (a[front] & 63) == 0
    last[front] = (a[front] & 63) == 63
    rest = ~(own | g0 | front)
    idx = g - 1
    i0 = rest & (idx == 0)
    cls[i0] = CLASSES.index("none_idx0")
    level[i0] = 1
    active = rest & ~i0
    L = 1
    while active.any():
        mult |= active & (idx % 64 == 0)
        hb = ((idx - 1) >> 6) << 6
        ent = np.where(a >= 0, a >> (6 * L), -1)
        assert (ent[active] < idx[active]).all()
        hit = active & (ent >= hb)
        cls[hit] = CLASSES.index("tree(%d)" % L)
        level[hit] = L
        first[hit] = ent[hit] == hb[hit]
        last[hit] = ent[hit] == idx[hit] - 1
        active &= ~hit
        z = active & (hb == 0)
        cls[z] = CLASSES.index("none_hb0")
        level[z] = L
        active &= ~z
        if L + 1 >= nlev:
            cls[active] = CLASSES.index("none_top")
            break
        idx = np.where(active, hb >> 6, idx)
        L += 1
    return c, a, cls, level, first, last, mult


def _level_sizes(n):
    sz, k = n, 1
    while sz > 64 and k < MAXLEV:
        sz = (sz + 63) // 64
        k += 1
        yield sz


def coverage(view):
    """Counter of (class, edge) over the live brackets of a document; edge "" counts the class itself.  Edges: c_lane0,
    c_lane63, a_lane0, a_lane63, hit_first, hit_last (entry hb / idx - 1 of the window of the hit; for group_in_front the
    window is the group), idx_mult64 (some window of the climb ended on a multiple of 64), and for a live close at depth 0
    root_odd / root_even (its tape offset) and root_open_first / root_open_last (its partner is the first / last bracket
    of its tile)."""
    a_all = view.answers()
    c, a, cls, level, first, last, mult = classify(view, a_all)
    cnt = collections.Counter()

    def add(mask, edge):
        for i, k in enumerate(np.bincount(cls[mask], minlength=len(CLASSES))):
            if k:
                cnt[(CLASSES[i], edge)] += int(k)

    add(np.ones(len(c), dtype=bool), "")
    add((c & 63) == 0, "c_lane0")
    add((c & 63) == 63, "c_lane63")
    add((a >= 0) & ((a & 63) == 0), "a_lane0")
    add((a >= 0) & ((a & 63) == 63), "a_lane63")
    add(first, "hit_first")
    add(last, "hit_last")
    add(mult, "idx_mult64")
    root = view.is_close[c] & (view.depth[c] == 0)
    add(root & (view.off[c] % 2 == 1), "root_odd")
    add(root & (view.off[c] % 2 == 0), "root_even")
    partner = a + 1  # (bracket 0 where there is no answer)
    tfirst = np.concatenate([[True], view.tile[1:] != view.tile[:-1]])
    tlast = np.concatenate([view.tile[1:] != view.tile[:-1], [True]])
    add(root & tfirst[partner], "root_open_first")
    add(root & tlast[partner], "root_open_last")
    return cnt


# ---- documents -------------------------------------------------------------------------------------------------------------
class _Builder:
    """valid JSON piece by piece: commas and (in an object) the key "k" come by themselves; nt / nb count the tokens and the
    brackets written so far"""

    def __init__(self):
        self.out = []
        self.stack = []
        self.nt = self.nb = 0

    def _lead(self):
        if not self.stack:
            return b""
        top = self.stack[-1]
        s = b"," if top[1] else b""
        top[1] += 1
        if top[0] == "obj":
            s += b'"k":'
        return s

    def _lead_tokens(self, s):
        return (1 if s.startswith(b",") else 0) + (2 if s.endswith(b":") else 0)

    def open(self, kind="arr"):
        s = self._lead()
        self.out.append(s + (b"{" if kind == "obj" else b"["))
        self.nt += self._lead_tokens(s) + 1
        self.nb += 1
        self.stack.append([kind, 0])

    def close(self):
        kind, _ = self.stack.pop()
        self.out.append(b"}" if kind == "obj" else b"]")
        self.nt += 1
        self.nb += 1

    def many(self, text, n, tokens, brackets):
        """n elements `text` (of `tokens` tokens and `brackets` brackets each)"""
        if n <= 0:
            return
        top = self.stack[-1]
        key = b'"k":' if top[0] == "obj" else b""
        el = b"," + key + text
        self.out.append((el if top[1] else key + text) + el * (n - 1))
        per = tokens + 1 + (2 if key else 0)
        self.nt += per * n - (0 if top[1] else 1)
        self.nb += brackets * n
        top[1] += n

    def pairs(self, n):
        self.many(b"[]", n, 2, 2)

    def zeros(self, n):
        self.many(b"0", n, 1, 0)

    def raw(self, text, tokens, brackets):
        self.many(text, 1, tokens, brackets)

    def close_all(self):
        while self.stack:
            self.close()

    def bytes(self):
        return b"".join(self.out)


def _zeros_to_seam(b, slack=2):
    """zeros so that the next token written lands `slack` or `slack + 1` tokens in front of the next tile seam"""
    per = 4 if b.stack[-1][0] == "obj" else 2
    room = (-b.nt) % S2_TILE - slack - 2
    if room < 0:
        room += S2_TILE
    b.zeros(room // per)


def far_pair_doc(n_between, a_indexes=(0,), kinds=("arr",), after=0, seam_behind_opener=False, bad_child=None,
                 bad_close=None):
    """Far containers inside one root array, nested in each other: container i opens at compact bracket index
    a_indexes[i] + 1, so the answer of its close and of every open among its direct children is bracket a_indexes[i]
    (pairs `[]` in front pad it there; an odd distance takes one more open bracket that stays open to the end).  The
    innermost holds n_between brackets (pairs `[]`: shallow, but deeper than the question), every outer one `after` pairs
    behind the inner close.  a_indexes = (): the root itself is the far container (no answer: bracket 0).
    seam_behind_opener: `0,` in front move the innermost open bracket to the end of its stage-2 tile, so that its first
    children are live although they sit in its group or the next one.
    bad_child = (i, j): child pair j of container i (i = -1: the root; behind the inner close for an outer one) comes without
    a key in an object, with a key in an array; bad_close = i: container i closes with the other kind of bracket.  Both
    are the only defect of the document, and only the lookup of that bracket's container can find it."""
    b = _Builder()
    b.open("arr")
    opened = [0]  # stack depth of every far container (the root first)
    for i, ai in enumerate(a_indexes):
        need = ai + 1 - b.nb
        assert need >= 0, (ai, b.nb)
        if need % 2:
            b.open("arr")
            need -= 1
        b.pairs(need // 2)
        if seam_behind_opener and i == len(a_indexes) - 1:
            _zeros_to_seam(b)
        assert b.nb == ai + 1
        b.open(kinds[i % len(kinds)])
        opened.append(len(b.stack) - 1)

    def children(i, n):
        top = b.stack[-1]
        if bad_child is not None and bad_child[0] == i:
            j = bad_child[1]
            b.pairs(j)
            if top[0] == "obj":  # a value without a key
                b.out.append(b",[]" if top[1] else b"[]")
            else:                # a key in an array
                b.out.append(b',"k":[]' if top[1] else b'"k":[]')
            top[1] += 1
            b.pairs(n - j - 1)
        else:
            b.pairs(n)

    def close(i):
        if bad_close == i:
            kind, _ = b.stack.pop()
            b.out.append(b"]" if kind == "obj" else b"}")
        else:
            b.close()

    children(len(a_indexes) - 1, n_between // 2)
    for i in range(len(a_indexes) - 1, -2, -1):
        while len(b.stack) - 1 > opened[i + 1]:
            b.close()
        if i < len(a_indexes) - 1:
            children(i, after)
        close(i)
    return b.bytes()


def excursion_doc(a_index, n_between, kind="arr"):
    """The answer behind a deep excursion: a container of pairs `[]` fills the compact indexes 1 .. a_index (2 .. with one
    more open bracket in front for an odd a_index) and its close bracket is the answer of the far container that opens
    right behind it.  Everything between the root's open bracket and the answer is deeper than the question, so in every
    window of every level the answer's entry is the ONLY one that qualifies: a minimum that tree12_body or k_min_upper
    gets wrong, or a descent that picks another entry, changes the partner."""
    b = _Builder()
    b.open("arr")
    if a_index % 2:
        b.open("arr")
    b.open("obj" if kind == "arr" else "arr")
    b.pairs((a_index - b.nb) // 2)
    b.close()
    assert b.nb == a_index + 1
    b.open(kind)
    b.pairs(n_between // 2)
    b.close_all()
    return b.bytes()


STAIR_GAPS = (0, 1, 0, 33, 0, 700, 2, 2300)


def staircase_doc(steps=136, gaps=STAIR_GAPS):
    """`steps` containers nested in each other (arrays and objects in turn) and closed by `steps` consecutive close
    brackets: every wave of the closes holds 64 distinct questions, all live (more than a tile of `0,` lies in the
    innermost container).  gaps[i % len] pairs `[]` in front of open bracket i spread the answers over groups, level-1
    windows and tiles."""
    b = _Builder()
    b.open("arr")
    for i in range(steps):
        b.pairs(gaps[i % len(gaps)])
        b.open("obj" if i % 2 else "arr")
    b.zeros(2200)
    b.close_all()
    return b.bytes()


COUNTS = (64, 65, 128, 4096, 4097, 4160, 262144, 262145)
LEVEL4_MIN = 64 ** 4 + 1


def count_doc(n_br):
    """exactly n_br brackets, one outermost pair around pairs `[]`: the questions of all the open brackets cross everything
    in front of them.  Brackets come in pairs: an odd n_br is only to be had with one close bracket too many (the last
    byte), and that document is rejected.  -> (bytes, valid)"""
    b = _Builder()
    b.open("arr")
    b.pairs((n_br - 2) // 2)
    b.close()
    doc = b.bytes()
    if n_br % 2:
        return doc + b"]", False
    return doc, True


def host_device_level_docs():
    """(a) more than 262144 tokens, 6002 brackets: the launcher, which only knows the tokens, sizes four levels and launches
    k_min_upper while the device's tree has three; (b) brackets just above 262144 (and tokens above that): four on both."""
    b = _Builder()
    b.open("arr")
    b.pairs(1500)
    b.zeros(135000)
    b.pairs(1500)
    b.close()
    return b.bytes(), count_doc(262144 + 258)[0]


def level4_doc():
    """The five-level tree (more than 64^4 brackets).  With 64^4 + 1 brackets the climb can not reach level 4: level 3
    then has 65 entries and the only window a climb forms there is [0, 64), which ends it (hb == 0).  A hit at level 4 needs
    a question from a bracket behind 65 * 64^3 + 2 * 64, and one that sweeps a level-1 window two 4096s more: the innermost of three far containers (answers at lane 0, lane 63
    and none) holds that many, and the children of the outer ones ask behind it."""
    n = 65 * 64 ** 3 + 3 * 64 * 64
    return far_pair_doc(n, a_indexes=(0, 63), kinds=("obj", "arr"), after=2100)


def _record(m, kind="arr", head=b""):
    """one record: `head` and m zeros in an array or an object"""
    if kind == "obj":
        return b"{" + head + b",".join([b'"k":0'] * m) + b"}"
    return b"[" + head + b",".join([b"0"] * m) + b"]"


def long_record_nd():
    """NDJSON whose long records (more than 4096 tokens: open and close bracket in different tiles, the root words written
    by k_br_match) alternate with records `[]`.  The long records begin at odd and at even tape offsets (an atom in front
    flips it), their open brackets are the last bracket of their tile, and -- after a record sized to end on a tile seam --
    the first one as well, once alone in the tile and once with more brackets behind it.
    -> (nd bytes, the same records as one plain array)"""
    recs = []
    tokens = [0]

    def add(r, t):
        recs.append(r)
        tokens[0] += t + 1  # + the separator

    def long_(kind="arr", head=b"", head_tokens=0):
        m = 2100 if kind == "arr" else 1100
        add(_record(m, kind, head), head_tokens + (2 * m + 1 if kind == "arr" else 4 * m + 1))

    def align():
        need = (-tokens[0]) % S2_TILE
        if need % 2:
            add(b"[]", 2)
            need = (-tokens[0]) % S2_TILE
        if need < 4:
            need += S2_TILE
        m = (need - 2) // 2
        add(_record(m), 2 * m + 1)
        assert tokens[0] % S2_TILE == 0

    long_()                                   # opens at token 0: first and last bracket of tile 0
    add(b"[]", 2)
    long_(head=b"true,", head_tokens=2)       # the next records begin one word later
    add(b"[]", 2)
    long_("obj")
    align()
    long_()                                   # opens on a tile seam
    add(b"[]", 2)
    align()
    long_(head=b"[],", head_tokens=3)         # first bracket of its tile, not the last
    add(b"[true]", 3)
    long_("obj", head=b'"k":null,', head_tokens=4)
    add(b"[]", 2)
    long_(head=b"[]," * 100, head_tokens=300)     # the partner of the close: a group or two in front
    long_(head=b"true,", head_tokens=2)
    long_(head=b"[]," * 3000, head_tokens=9000)   # ... and beyond the level-1 window
    long_()
    return b"\n".join(recs), b"[" + b",".join(recs) + b"]"


def small_far_docs():
    """name -> document: the far containers at the group, window and tile edges (all under 100 KB)"""
    docs = {}
    for ai in (0, 10, 11, 63, 64, 127, 128):
        for kind in ("arr", "obj"):
            docs["seam_a%d_%s" % (ai, kind)] = far_pair_doc(400, (ai,), (kind,), seam_behind_opener=True)
    for ai in (0, 63, 64, 4095, 4096, 8191):
        for kind in ("arr", "obj"):
            docs["far_a%d_%s" % (ai, kind)] = far_pair_doc(13000, (ai,), (kind,))
    # the answer alone in its window, in each quarter of a level-2 entry (one wave of tree12_body each), lanes 0 and 63
    for ai in (4096 + 10, 4096 + 1024 + 63, 4096 + 2048, 4096 + 3072, 8191):
        docs["excursion_a%d" % ai] = excursion_doc(ai, 13000, "obj" if ai % 2 else "arr")
    docs["far_nested"] = far_pair_doc(9000, (0, 63, 4160, 4223), ("arr", "obj"), after=4300)
    docs["far_root"] = far_pair_doc(9000, ())
    return docs


def big_far_docs():
    """the documents that reach level 3 of the tree (answers at lane 0 and lane 63, both kinds of container)"""
    n = 65 * 64 * 64 + 3 * 64 * 64
    return {"excursion3": excursion_doc(64 ** 3 + 3 * 4096 + 63, 64 ** 3 + 6 * 4096),  # level 3, its entry 1
            "far3_arr_obj": far_pair_doc(n, (0, 63), ("arr", "obj"), after=4300),
            "far3_obj_arr": far_pair_doc(n, (0, 63), ("obj", "arr"), after=4300)}


def valid_docs():
    """name -> (document, nd) of every valid document but the level-4 one"""
    docs = {k: (v, False) for k, v in small_far_docs().items()}
    docs.update({k: (v, False) for k, v in big_far_docs().items()})
    docs["staircase"] = (staircase_doc(), False)
    for n in COUNTS:
        d, ok = count_doc(n)
        if ok:
            docs["count_%d" % n] = (d, False)
        else:  # the valid neighbour: the same level sizes
            docs["count_%d" % (n + 1)] = (count_doc(n + 1)[0], False)
    a, b = host_device_level_docs()
    docs["levels_host4_device3"] = (a, False)
    docs["levels_both4"] = (b, False)
    nd, plain = long_record_nd()
    docs["long_records_nd"] = (nd, True)
    docs["long_records_plain"] = (plain, False)
    return docs


def error_docs():
    """name -> rejected document: one defect each, which only a far lookup finds"""
    docs = {}
    for n in COUNTS:
        d, ok = count_doc(n)
        if not ok:
            docs["count_%d_one_close_too_many" % n] = d
    for kind in ("arr", "obj"):
        docs["close_kind_%s" % kind] = far_pair_doc(13000, (63,), (kind,), bad_close=0)        # answered through the tree
        docs["child_%s" % kind] = far_pair_doc(13000, (63,), (kind,), bad_child=(0, 6400))
        docs["seam_child_%s" % kind] = far_pair_doc(400, (10,), (kind,), seam_behind_opener=True, bad_child=(0, 20))
        docs["seam_close_%s" % kind] = far_pair_doc(400, (63,), (kind,), seam_behind_opener=True, bad_close=0)
    n3 = 65 * 64 * 64 + 3 * 64 * 64
    docs["far3_outer_child"] = far_pair_doc(n3, (0, 63), ("obj", "arr"), after=4300, bad_child=(0, 4200))
    docs["far3_outer_close"] = far_pair_doc(n3, (0, 63), ("arr", "obj"), after=4300, bad_close=0)
    docs["far3_inner_close"] = far_pair_doc(n3, (0, 63), ("arr", "obj"), after=4300, bad_close=1)
    # no answer at all (bracket 0): the root closes with the wrong kind, a key in the root array far behind its open
    docs["root_close_kind"] = far_pair_doc(9000, (), bad_close=-1)
    docs["root_child"] = far_pair_doc(9000, (), bad_child=(-1, 4400))
    docs["root_close_kind_count_4160"] = count_doc(4160)[0][:-1] + b"}"
    return docs
