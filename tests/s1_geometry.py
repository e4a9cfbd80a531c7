"""Where stage 1 and stage 2 cut a message, and documents that put a hazard exactly on those cuts.  No GPU import.

Stage 1 (csrc/stage1.hip s1_plan, TileMap, tile_unit) splits the 4 KiB units of a message -- unit u holds the bytes
[4096 u, 4096 u + 4096) of (lead + message), lead = the pointer's offset in its 64-byte line -- into whole rounds of
full tiles (`per_tile` units each, one tile per block slot) and then one short round of small tiles of `su` units.
Two folds turn the units behind the whole rounds into more full tiles instead: when `su` would not be smaller than a
full tile, and when fewer units than block slots follow at least one whole round.  A plan of more tiles than blocks
draws every tile from a ticket counter (stage1_kernel: one_round).  Stage 2 cuts the structural indexes into tiles
of S2_TILE = 4096 tokens (csrc/stage2.hip).

plan() mirrors s1_plan, seams() names the byte offsets of every kind of cut, byte_doc() and token_doc() build valid
documents (plain JSON or NDJSON) with a hazard at a chosen byte offset or structural index.  tests/test_s1_geometry.py
checks on the CPU that the documents are what they claim; tests/test_gpu_seams.py runs them on the device."""
import collections

import numpy as np

UNIT = 4096
S2_TILE = 4096

# csrc/stage1.hip S1_VARIANTS: (block, ch, wpe, depth); a tile is block / 64 * ch units
S1_VARIANTS = [(512, 2, 4, 0), (1024, 2, 4, 0), (768, 2, 3, 0), (1024, 2, 4, 2), (1024, 2, 4, 3), (1024, 1, 4, 0)]
DEFAULT_VARIANT = 1
MI355X_CUS = 256

Plan = collections.namedtuple("Plan", "variant cus per_tile slots nu nf su tiles one_round branch")


def per_tile(variant):
    block, ch, _, _ = S1_VARIANTS[variant]
    return block // 64 * ch


def slots(variant, cus):
    return cus * (2 if S1_VARIANTS[variant][0] <= 512 else 1)  # s1_block_slots: 16 waves per CU


def units_of(length, lead):
    return (lead + length + UNIT - 1) // UNIT


def plan(length, lead, variant, cus=MI355X_CUS):
    """s1_plan(len, lead) for `variant` on a device of `cus` compute units."""
    P, S = per_tile(variant), slots(variant, cus)
    nu = units_of(length, lead)
    nf = nu // (P * S) * S
    rest = nu - nf * P
    su = (rest + S - 1) // S
    branch = "rounds" if nf and rest == 0 else ("tail" if nf else "small")
    if su >= P or (nf > 0 and rest < S):
        if rest:
            branch = "fold_big_su" if su >= P else "fold_few_units"
        nf += (rest + P - 1) // P
        rest = 0
        su = P
    su = max(su, 1)
    tiles = nf + (rest + su - 1) // su
    return Plan(variant, cus, P, S, nu, nf, su, tiles, tiles <= S, branch)


def tile_unit(p, t, local, units_per_tile=None):
    """tile_unit<UNITS>(tm, t, local) of the kernel: the unit a tile's `local`-th slot holds, or None (void).
    units_per_tile: the kernel's UNITS (default: the plan's own)."""
    K = p.per_tile if units_per_tile is None else units_per_tile
    if t < p.nf:
        u = t * K + local
    elif local < p.su:
        u = p.nf * K + (t - p.nf) * p.su + local
    else:
        return None
    return u if u < p.nu else None


def tile_units(p, units_per_tile=None):
    """per tile the list of units it holds (void slots left out), in tile order"""
    K = p.per_tile if units_per_tile is None else units_per_tile
    out = []
    for t in range(p.tiles):
        us = [tile_unit(p, t, k, K) for k in range(K)]
        out.append([u for u in us if u is not None])
    return out


def tile_starts(p):
    """first unit of every tile (the plan's own shape)"""
    return [t * p.per_tile if t < p.nf else p.nf * p.per_tile + (t - p.nf) * p.su for t in range(p.tiles)]


SEAM_CLASSES = ("unit_full", "unit_small", "small", "full", "full_small", "last_tile", "end")


def seams(length, lead, variant, cus=MI355X_CUS):
    """message byte offsets of every kind of cut of the plan (each offset is the first byte behind the cut):
    unit_full / unit_small: unit seams inside a full / small tile; small / full: seams between two small / two full
    tiles; full_small: the seam between the last full and the first small tile; last_tile: where the last tile
    begins; end: the message end (= length)."""
    p = plan(length, lead, variant, cus)
    starts = tile_starts(p)
    out = {k: [] for k in SEAM_CLASSES}

    def off(u):
        return u * UNIT - lead

    for t, s in enumerate(starts):
        full = t < p.nf
        n = p.per_tile if full else p.su
        for k in range(1, n):
            if s + k < p.nu:
                out["unit_full" if full else "unit_small"].append(off(s + k))
        if t == 0 or s >= p.nu:
            continue
        if full:
            out["full"].append(off(s))
        elif t == p.nf:
            out["full_small"].append(off(s))
        else:
            out["small"].append(off(s))
    if p.tiles > 1 and starts[-1] < p.nu:
        out["last_tile"].append(off(starts[-1]))
    out["end"].append(length)
    return p, out


def branch_units(variant, cus=MI355X_CUS):
    """unit counts that take every branch of the plan for `variant`: name -> units"""
    P, S = per_tile(variant), slots(variant, cus)
    R = P * S
    return {
        "one_unit": 1,
        "less_than_slots": S - 1,
        "small_tiles_one_each": S + 1,
        "su_per_tile_minus_1": S * (P - 1),          # su == UNITS - 1, tiles == slots
        "su_fold": S * (P - 1) + 1,                 # su >= UNITS: full tiles
        "one_round": R,                              # tiles == slots (one round: static tiles)
        "round_plus_1": R + 1,                       # fewer units than slots behind it: folded, slots + 1 tiles (tickets)
        "round_plus_slots_minus_1": R + S - 1,
        "round_plus_slots": R + S,                   # a tail of small tiles of one unit
        "round_plus_2_slots_plus_1": R + 2 * S + 1,  # small tiles of three units
        "two_rounds": 2 * R,
    }


def all_tail_units(cus=MI355X_CUS, variants=None):
    """the smallest unit count whose plan has a tail of small tiles of at least 2 units for every variant: a message of
    that size has every seam class of every variant"""
    variants = range(len(S1_VARIANTS)) if variants is None else variants
    n = max(per_tile(v) * slots(v, cus) for v in variants) + 1
    while True:
        ps = [plan(n * UNIT, 0, v, cus) for v in variants]
        if all(p.branch == "tail" and 2 <= p.su < p.per_tile for p in ps):
            return n
        n += 1


# ---- hazards ---------------------------------------------------------------------------------------------------------
# name -> fn(nd) -> (text, anchor, structural): `text` is one array element (or, for the ND separator, the end of one
# record and the start of the next); text[anchor] is the byte placed at seam + shift; `structural` says whether the
# oracle's stage 1 reports that byte.
def _h(text, anchor, structural):
    return lambda nd: (text, anchor, structural)


HAZARDS = {
    # backslash runs in front of a quote; the anchor is the ']' right behind the quote: a structural only if the quote
    # closed the string (a closing quote is never a structural itself)
    "bs_odd_1": _h(b'["ab\\"]"]', 6, False),
    "bs_even_2": _h(b'["ab\\\\"]', 7, True),
    "bs_odd_3": _h(b'["a\\\\\\"]"]', 7, False),
    "bs_even_64": _h(b'["' + b"\\" * 64 + b'"]', 67, True),     # runs longer than a 64-byte chunk
    "bs_odd_65": _h(b'["' + b"\\" * 65 + b'"]"]', 68, False),
    "escaped_quote": _h(b'"\\""', 1, False),                    # the backslash on the seam
    "string_across": _h(b'"' + b"x" * 40 + b",:{" + b"y" * 40 + b'"', 41, False),  # opens before, closes after
    "u_escape": _h(b'"\\u00e9\\u20ac"', 7, False),
    "surrogate_pair": _h(b'"\\ud83d\\ude00"', 7, False),        # the seam between the two halves
    "slow_float": _h(b"2.2250738585072011e-308", 11, False),     # straddles the seam; needs the exact path
    "int20": _h(b"18446744073709551616", 10, False),             # 2^64: a float in the reference
    "int64_min": _h(b"-9223372036854775808", 10, False),
    "true": _h(b"true", 2, False),
    "null": _h(b"null", 2, False),
    "brackets": _h(b"[{}]", 1, True),
    # a raw newline: whitespace in a plain document, a record separator (and a structural) in NDJSON
    "newline": lambda nd: (b"0]\n[0", 2, True) if nd else (b"0,\n 0", 2, False),
}
# a string with a control character: stage 1 rejects the document
ERROR_HAZARDS = {"control_in_string": _h(b'"a\x01b"', 2, False)}
ALL_HAZARDS = dict(HAZARDS, **ERROR_HAZARDS)
SHIFTS = (-3, -2, -1, 0, 1, 2)  # -2..+2 around the seam; -3 too, so that a document built for lead 0 serves lead 1


def combos():
    return [(h, s) for h in HAZARDS for s in SHIFTS]


Target = collections.namedtuple("Target", "offset hazard shift")
Placed = collections.namedtuple("Placed", "target start anchor_at structural")


def _sep(nd):
    return b"]\n[" if nd else b","


def place(length, targets, nd=False):
    """the targets byte_doc() keeps, in byte order: a target that does not fit (overlaps the one before, or the ends of
    the message) is left out.  -> list of Placed"""
    sep = _sep(nd)
    placed = []
    free = 1  # first byte a text may use
    for tg in sorted(targets, key=lambda x: x.offset + x.shift):
        text, anchor, structural = ALL_HAZARDS[tg.hazard](nd)
        start = tg.offset + tg.shift - anchor
        if start < free or start + len(text) > length - 1:
            continue
        placed.append(Placed(tg, start, tg.offset + tg.shift, structural))
        free = start + len(text) + len(sep)
    return placed


def byte_doc(length, targets, nd=False):
    """A valid document of exactly `length` bytes with, for every target, text[anchor] of its hazard at
    offset + shift.  Plain: one array ``[ e0, e1, ... ]``; nd: one record ``[ e ]`` per element.  The rest is blanks,
    so every offset is exact.  -> (numpy uint8 array, list of Placed)"""
    sep = np.frombuffer(_sep(nd), dtype=np.uint8)
    a = np.full(length, 0x20, dtype=np.uint8)
    a[0], a[length - 1] = ord("["), ord("]")
    placed = place(length, targets, nd)
    for i, pl in enumerate(placed):
        text = ALL_HAZARDS[pl.target.hazard](nd)[0]
        e = pl.start + len(text)
        a[pl.start:e] = np.frombuffer(text, dtype=np.uint8)
        if i + 1 < len(placed):
            a[e:e + sep.size] = sep
    return a, placed


def rotation_targets(length, lead, k, cus=MI355X_CUS):
    """one target on EVERY unit seam of a message at `lead` (which covers the seams of every class of every variant),
    combination (unit + k) mod len(combos()) of hazard and shift: over k = 0 .. len(combos()) - 1 every seam carries
    every combination once"""
    cs = combos()
    n = units_of(length, lead)
    out = []
    for u in range(1, n):
        h, s = cs[(u + k) % len(cs)]
        out.append(Target(u * UNIT - lead, h, s))
    return out


def message_end_targets(length, k):
    """a hazard that ends 0 .. 5 bytes in front of the closing bracket of the message"""
    cs = combos()
    h, s = cs[k % len(cs)]
    text, anchor, _ = HAZARDS[h](False)
    return Target(length - 1 - (s + 3) - len(text) + anchor, h, 0)


def seam_doc_length(cus=MI355X_CUS):
    """length of the byte-seam documents: every seam class of every variant, at every lead 0..63"""
    n = all_tail_units(cus)
    return (n - 1) * UNIT + 1500


def byte_seam_doc(k, lead, nd, cus=MI355X_CUS):
    """document k of the rotation for messages at `lead` (and lead + 1: SHIFTS reaches -3)"""
    length = seam_doc_length(cus)
    tg = rotation_targets(length, lead, k, cus)
    tg.append(message_end_targets(length, k))
    return byte_doc(length, tg, nd)


def sparse_doc(length, lead, variants, cus=MI355X_CUS, hazard="string_across", nd=False):
    """blanks everywhere but on the cuts that occur once per plan (full/small seam, last tile), the first and last few
    seams of the other classes: units without a single structural, blank runs far longer than a unit"""
    tg = []
    for v in variants:
        _, sm = seams(length, lead, v, cus)
        for cls in ("full_small", "last_tile"):
            tg += [Target(o, hazard, 0) for o in sm[cls]]
        for cls in ("small", "full", "unit_small"):
            tg += [Target(o, hazard, 0) for o in sm[cls][:2] + sm[cls][-2:]]
    uniq = {t.offset: t for t in tg}
    return byte_doc(length, list(uniq.values()), nd)


# ---- token seams (stage 2: S2_TILE tokens per tile) ---------------------------------------------------------------------
# kind -> (text, anchor): text[anchor] is the structural placed at index 4096 t + d; nd-only kinds need NDJSON
TOKEN_KINDS = {
    "bracket_split": (b"[]", 0),         # '[' and ']' on the two sides of the seam (d = -1), or both behind it
    "brace_split": (b"{}", 0),
    "key_colon_value": (b'{"key":"value"}', 1),
    "key_colon_value@colon": (b'{"key":"value"}', 6),
    "escaped_string": (b'"a\\"b\\\\c\\u00e9\\n"', 0),
    "int64_min": (b"-9223372036854775808", 0),
    "uint64_overflow": (b"18446744073709551616", 0),
    "true": (b"true", 0),
    "false": (b"false", 0),
    "null": (b"null", 0),
    "nd_separator": (b"0]\n[0", 2),
}
ND_ONLY = {"nd_separator"}
TOKEN_OFFSETS = (-1, 0, 1)


def _tokens_before(text, anchor, nd, oracle_stage1):
    """structurals of `text` (as an array element) in front of text[anchor], and in all"""
    ok, pos = oracle_stage1(b"[" + text + b"]", nd)
    assert ok, text
    pos = [int(p) - 1 for p in pos[1:-1]]
    assert anchor in pos, (text, anchor)
    return pos.index(anchor), len(pos)


def _filler(n):
    """exactly n structurals (n == 0 or n >= 2) as array elements, each followed by a comma"""
    assert n == 0 or n >= 2, n
    if n % 2:
        return b"[]," + b"0," * ((n - 3) // 2)
    return b"0," * (n // 2)


def token_doc(kind, d, oracle_stage1, tiles=(1, 2, 3), tail=1500, nd=False):
    """A valid document whose hazard `kind` has its anchor structural at stage-1 index 4096 t + d for t in `tiles`; the
    last entry of `tiles` is the last stage-2 tile (the document ends `tail` structurals behind it).
    -> (bytes, [structural index of every anchor], [byte offset of every anchor])"""
    text, anchor = TOKEN_KINDS[kind]
    nd = nd or kind in ND_ONLY
    before, total = _tokens_before(text, anchor, nd, oracle_stage1)
    out = bytearray(b"[")
    count = 1
    idx, offs = [], []
    for t in tiles:
        want = S2_TILE * t + d - before  # index of the element's first structural
        gap = want - count
        if gap == 1:  # (never for these tiles: the first gap is large and the elements are far apart)
            raise AssertionError("cannot place one structural")
        out += _filler(gap)
        count += gap
        offs.append(len(out) + anchor)
        idx.append(count + before)
        out += text + b","
        count += total + 1
    out += _filler(max(tail, 2) // 2 * 2) + b"0]"
    assert (count + tail // 2 * 2 + 2 - 1) // S2_TILE == tiles[-1]
    return bytes(out), idx, offs


def nesting_doc(depth):
    return b"[" * depth + b"]" * depth
