"""The device's segmented reduction (agg_layout, k_q_agg_heads, k_q_agg_rows' flags, agg_tile and the fold loop of agg_enqueue,
csrc/query.hip), restated on lists -- the host model of its geometry (test infrastructure, like batch_geometry.py and
ser_geometry.py).  aggregate_walk.reduce says WHAT an aggregate is; this file says in which tiles, slots and levels the device
gets there, and in which association, so that a case can prove it lies on the seam it is named for and a float sum can be held
to its bits.

Geometry.  Rows are reduced in tiles of AGG_TILE = 256; a tile hands at most two items to the next level -- slot A, the piece of
a segment that began in an earlier tile, slot B, the piece of the segment left open at the tile's end --, AGG_TILE items make a
tile of the next level, and the levels repeat until one fits a single tile:
  levels(n)            the tiles of every level (agg_layout): 1 level up to 256 rows, 2 up to ROWS_PER_FOLD_TILE, 3 up to
                       ROWS_PER_FOLD2_TILE, then 4
  ROWS_PER_FOLD_TILE   the rows below one tile of level 1: AGG_TILE / 2 row tiles (two slots each) of AGG_TILE rows = 32 768
  ROWS_PER_FOLD2_TILE  the rows below one tile of level 2: 128 times that

The reduction.  An item is (v, rec1, flags): v = (ok, bad, s0, s1, mn, mx) as AggVal -- FLOAT: s0 a Python float (IEEE double
addition, identity -0.0); INT / UINT: s0, s1 the sums of the low and of the high 32-bit halves modulo 2^64, put together as 128
bits where a segment is stored; mn, mx keys (aggregate_walk.key) --, rec1 the record + 1 of a head, flags of VALID, HEAD, END.
  tile(items, kind)    one block of agg_tile in the device's order of joins: the 64-lane scan in steps 1, 2, 4 ... 32 joins
                       (lane - s, lane) for lane >= s unless the lane's partial already starts at a head, then the waves in wave
                       order through the tails; an item that is not VALID carries the identity and is transparent
                       -> (the segments stored [(record, v)], slot A, slot B); an empty slot is NONE
  run(values, statuses, offsets, kind, one_segment)
                       the rows' items (offsets None: record r owns row r and is stored as it is, AGG_OWN; one_segment: one
                       record over all rows, AGG_ONE; else the heads of k_q_agg_heads, AGG_OFFS), tile after tile, level after
                       level -> (the six per-record arrays as bit patterns, Trace)
  Trace                .tiles = levels(n); .stored[record] = the level that stored it; .items[level] = the (tile, slot, flags)
                       of every item that level produced (slot "A" / "B"; empty slots are left out)
`mutant` names one deliberate mistake (MUTANTS); tests/test_agg_geometry.py asserts that the case lists below tell every one of
them from the reduction.

Case lists: Case(name, claim, rows, pattern, own) -- rows: the rows of every record; pattern: how texts() fills them; own: the
records are the rows (no selection: AGG_OWN per record, AGG_ONE for the total); claim: what the trace must show (holds()).
Every list uses the smallest sizes that reach its seam.  Pinned by tests/test_agg_geometry.py; run on the device by
tests/test_gpu_aggregate_seams.py."""
import collections
import functools
import random

import aggregate_walk as AW
import column_walk as CW

AGG_TILE = AW.AGG_TILE
T = AGG_TILE
ROWS_PER_FOLD_TILE = AGG_TILE * AGG_TILE // 2
ROWS_PER_FOLD2_TILE = ROWS_PER_FOLD_TILE * (AGG_TILE // 2)
F = ROWS_PER_FOLD_TILE
VALID, HEAD, END = 1, 2, 4
U64 = (1 << 64) - 1
FLOAT, INT, UINT = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT

MUTANTS = ("identity +0.0", "empty slot is a head", "invalid last thread drops B", "tails without the head stop", "slot A without END",
           "o and v swapped")


def levels(n):
    """the tiles of every level of n rows (> 0), as agg_layout gives them"""
    out, m = [], n
    while True:
        tiles = (m + AGG_TILE - 1) // AGG_TILE
        out.append(tiles)
        if tiles == 1:
            return out
        m = 2 * tiles


def identity(kind, mutant=None):
    zero = (0.0 if mutant == "identity +0.0" else -0.0) if kind == FLOAT else 0
    return (0, 0, zero, 0, U64, 0)


def join(a, b, kind):
    """a: the rows in front, b: the rows behind (agg_join)"""
    s0 = a[2] + b[2] if kind == FLOAT else (a[2] + b[2]) & U64
    return (a[0] + b[0], a[1] + b[1], s0, (a[3] + b[3]) & U64, a[4] if a[4] < b[4] else b[4], a[5] if a[5] > b[5] else b[5])


def row_value(bits, status, kind):
    """the partial a lane of k_q_agg_rows leaves for one row"""
    if status != CW.COL_OK:
        return (0, 1) + identity(kind)[2:]
    k = AW.key(bits, kind)
    if kind == FLOAT:
        return (1, 0, CW.bits2f(bits), 0, k, k)
    hi = bits >> 32
    if kind == INT and bits >> 63:
        hi |= 0xFFFFFFFF00000000  # (the high half signed)
    return (1, 0, bits & 0xFFFFFFFF, hi, k, k)


def stored_arrays(v, kind):
    """(count, not_ok, sum lo, sum hi, min, max) of a finished segment, as agg_store writes them"""
    lo = hi = 0
    if v[0]:
        if kind == FLOAT:
            lo = CW.f2bits(v[2])
        else:  # s0 + s1 * 2^32 in 128 bits
            lo = (v[2] + (v[3] << 32)) & U64
            top = v[3] >> 32
            if kind == INT and v[3] >> 63:
                top |= 0xFFFFFFFF00000000
            hi = (top + (1 if lo < v[2] else 0)) & U64
    unkey = lambda k: AW.key(k, kind) if kind != FLOAT else ((~k & U64) if not k >> 63 else k ^ (1 << 63))  # noqa: E731
    return (v[0], v[1], lo, hi, unkey(v[4]) if v[0] else 0, unkey(v[5]) if v[0] else 0)


def NONE(kind, mutant=None):
    return (identity(kind, mutant), 0, 0)


def _merge(st, ost):
    return ((st | ost) & 1) | ((st & 6) or (ost & 6))


def tile(items, kind, mutant=None):
    """one block of agg_tile over up to AGG_TILE items (v, rec1, flags) -> (stored [(record, v)], slot A, slot B)"""
    assert 0 < len(items) <= AGG_TILE
    none = NONE(kind, mutant)
    items = list(items) + [none] * (AGG_TILE - len(items))
    v = [it[0] if it[2] & VALID else none[0] for it in items]
    rk = [it[1] for it in items]
    valid = [bool(it[2] & VALID) for it in items]
    end = [bool(it[2] & VALID and it[2] & END) for it in items]
    st = [(1 if it[2] & HEAD else 0) | ((4 if it[2] & END else 2) if it[2] & VALID else 0) for it in items]
    if mutant == "empty slot is a head":
        st = [s | (0 if ok else 1) for s, ok in zip(st, valid)]
    swapped = mutant == "o and v swapped"
    stored, slot_a, slot_b = [], none, none
    acc, ast, ark = identity(kind, mutant), 0, 0  # the waves in front, joined in wave order through their tails
    for w0 in range(0, AGG_TILE, 64):
        wv, wst, wrk = v[w0:w0 + 64], st[w0:w0 + 64], rk[w0:w0 + 64]
        s = 1
        while s < 64:  # the scan of the wave: every lane >= s takes the lane s in front of it, all at once
            nv, nst, nrk = wv[:], wst[:], wrk[:]
            for i in range(s, 64):
                o = i - s
                if swapped:  # the lane in front is taken for the one behind: its head stops the join
                    if not wst[o] & 1:
                        nv[i] = join(wv[i], wv[o], kind)
                elif not wst[i] & 1:
                    nv[i] = join(wv[o], wv[i], kind)
                nst[i] = _merge(wst[i], wst[o])
                if wrk[o] > wrk[i]:
                    nrk[i] = wrk[o]
            wv, wst, wrk = nv, nst, nrk
            s <<= 1
        for lane in range(64):
            i = w0 + lane
            x = wv[lane] if wst[lane] & 1 else join(acc, wv[lane], kind)
            s = _merge(wst[lane], ast)
            r = max(wrk[lane], ark)
            f, is_open, last = bool(s & 1), s & 6 == 2, i == AGG_TILE - 1
            if end[i] and f:
                stored.append((r - 1, x))
            if not f and (end[i] or (last and is_open)):
                slot_a = (x, 0, VALID | (END if end[i] and mutant != "slot A without END" else 0))
            if f and last and is_open and (valid[i] or mutant != "invalid last thread drops B"):
                slot_b = (x, r, VALID | HEAD)
        t = (wv[63], wrk[63], wst[63])  # s_tail[wave]
        acc = t[0] if t[2] & 1 and mutant != "tails without the head stop" else join(acc, t[0], kind)
        ast = _merge(t[2], ast)
        ark = max(ark, t[1])
    return stored, slot_a, slot_b


class Trace:
    def __init__(self, tiles):
        self.tiles, self.stored, self.items = tiles, {}, []


def run(values, statuses, offsets, kind, one_segment=False, mutant=None):
    """-> ((count, not_ok, sum lo, sum hi, min, max) as lists of uint64 patterns, one entry per record; Trace)"""
    n = len(values)
    assert len(statuses) == n
    rows = [row_value(b, st, kind) for b, st in zip(values, statuses)]
    if one_segment:
        records, offsets = 1, [0, n]
    elif offsets is None:  # AGG_OWN: record r owns row r and is stored as it is
        out = [list(col) for col in zip(*[stored_arrays(v, kind) for v in rows])] if n else [[] for _ in range(6)]
        trace = Trace([(n + AGG_TILE - 1) // AGG_TILE])
        trace.stored = {r: 0 for r in range(n)}
        return tuple(out), trace
    else:
        records = len(offsets) - 1
        assert offsets[0] == 0 and offsets[-1] == n
    out = tuple([0] * records for _ in range(6))
    if n == 0:  # nothing is launched: the outputs stay 0
        return out, Trace([])
    head = [0] * (n + 1)
    for r in range(records):  # k_q_agg_heads
        if offsets[r + 1] > offsets[r]:
            head[offsets[r]] = r + 1
    head[n] = 1  # (r + 1 == n ends the last segment)
    below = [(v, head[r], VALID | (HEAD if head[r] else 0) | (END if head[r + 1] else 0)) for r, v in enumerate(rows)]
    trace = Trace(levels(n))
    for level, tiles in enumerate(trace.tiles):
        assert tiles == (len(below) + AGG_TILE - 1) // AGG_TILE
        items, produced = [], []
        for b in range(tiles):
            stored, slot_a, slot_b = tile(below[b * AGG_TILE:(b + 1) * AGG_TILE], kind, mutant)
            for rec, v in stored:
                if 0 <= rec < records:  # (a mutant may store at no record at all)
                    trace.stored[rec] = level
                    for dst, x in zip(out, stored_arrays(v, kind)):
                        dst[rec] = x
            for slot, it in (("A", slot_a), ("B", slot_b)):
                if it[2]:
                    produced.append((b, slot, it[2]))
            items += [slot_a, slot_b]
        trace.items.append(produced)
        below = items
    return out, trace


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
class Case(collections.namedtuple("Case", "name claim rows pattern own")):
    __slots__ = ()

    def __hash__(self):  # (the claim is a dict; a case is told by the rest)
        return hash((self.name, self.rows, self.pattern, self.own))
SEED = 20260


def _c(name, claim, rows, pattern="ints", own=False):
    return Case(name, claim, tuple(rows), pattern, own)


def level_counts():
    """the seams between 1, 2 and 3 levels: 256 | 257 rows and F | F + 1 rows (F itself fills one tile of level 1 exactly)"""
    out = []
    for n in (1, 63, 64, 65, 255, 256, 257):
        lv = 1 if n <= T else 2
        out.append(_c("one record of %d rows" % n, {"levels": lv, "stored": {0: lv - 1}}, [n]))
        out.append(_c("%d one-row records" % n, {"levels": lv, "own": True}, [1] * n, own=True))
    for n in (F - 1, F, F + 1, F + 255, F + 256, F + 257):
        lv = 2 if n <= F else 3
        claim = {"levels": lv, "stored": {0: lv - 1}}
        if n > F:  # the second tile of level 1 holds the slots of 1, 1, 2 and 3 row tiles
            claim["tiles"] = [(n + T - 1) // T, 2, 1]
        out.append(_c("one record of %d rows" % n, claim, [n]))
    return out


def fold_shapes():
    """(name, claim, rows) of the shapes that lie on the seams of the tiles of level 1; three levels each"""
    n2 = F + 2 * T + 3
    out = []
    for cut, what in ((F - T, "F - T"), (F - 1, "F - 1"), (F, "F"), (F + 1, "F + 1"), (F + T, "F + T")):
        claim = {"levels": 3, "cut": cut, "stored": {0: 1 if cut <= F else 2, 1: 2 if cut < F else 1}}
        if cut == F - T:  # the second record owns the whole last row tile of fold tile 0: its B item is the tile's last item
            claim["b_at_255"] = True
        if cut in (F + 1, F + T):  # the first record ends in the first row tile of fold tile 1 (F + T: on its edge)
            claim["a_end_first_slot"] = True
        out.append(("two records cut at " + what, claim, [cut, n2 - cut]))
    start = F - T + 7  # inside the last row tile of fold tile 0
    for end, what in ((F + 9, "in the first row tile"), (F + 3 * T + 9, "after three whole row tiles"), (F + 2 * T, "on a tile edge")):
        claim = {"levels": 3, "b_at_255": True, "stored": {0: 1, 1: 2, 2: 1}}
        if end == F + 9:
            claim["a_end_first_slot"] = True
        else:
            claim["a_open_first_slot"] = True
        out.append(("a record from the last row tile of fold tile 0, ending " + what, claim, [start, end - start, T + 3]))
    # from row tile 125 of fold tile 0 over all of fold tile 1 into fold tile 2: slot A of fold tile 1 stays open, the B item of
    # fold tile 0 comes from a last thread that is not VALID (the empty slot B of row tile 127), and level 2 reads A and B items
    out.append(("a record over three fold tiles",
                {"levels": 3, "tiles": [259, 3, 1], "a_open_whole_tile": 1, "b_from_invalid_last": True, "second_fold_ab": True,
                 "stored": {0: 1, 1: 2, 2: 1}},
                [F - 2 * T - 5, F + 3 * T + 16, T - 9]))
    # a head in the second wave of a row tile AND of a fold tile, its segment running on through the waves behind it: the only
    # place where the join of the wave tails has a head to stop at with something in front of it
    out.append(("a record from the second wave of a row tile and of a fold tile through the waves behind",
                {"levels": 3, "head_in_wave": 1, "stored": {0: 2, 1: 1, 2: 0}}, [F + 40 * T + 100, 60 * T, 7]))
    out.append(("records without rows at 0, F and n", {"levels": 3, "empty_at": (0, F, F + T + 3), "stored": {3: 1, 6: 1}},
                [0, 0, 0, F, 0, 0, T + 3, 0, 0]))
    out.append(("one-row records on both sides of row F", {"levels": 3, "stored": {0: 1, 1: 0, 2: 0, 3: 0, 4: 0, 5: 1}, "heads_at": (F - 2, F - 1, F, F + 1)},
                [F - 2, 1, 1, 1, 1, T + 3]))
    return out


THREE = "a record over three fold tiles"
CUT = "two records cut at F + 1"


def fold_seams():
    out = [_c(name, claim, rows) for name, claim, rows in fold_shapes()]
    n = F + T + 3
    out.append(_c("%d one-row records under a selection" % n, {"levels": 3, "all_at_level": 0, "no_items": True}, [1] * n))
    out.append(_c("%d one-row records" % n, {"levels": 3, "own": True}, [1] * n, own=True))
    return out


def statuses():
    out = [_c(name + ", every 11th row not OK", claim, rows, "ints/11") for name, claim, rows in fold_shapes()]
    out.append(_c("a whole row tile of rows that are not OK inside a record", {"levels": 2, "bad_tile": 2, "stored": {0: 0, 1: 1, 2: 0}},
                  [5, 4 * T, 3], "ints/tile2"))
    out.append(_c("a record of more than 2 T rows without an OK row", {"levels": 2, "all_zero": 1, "stored": {0: 0, 1: 1, 2: 1}},
                  [9, 2 * T + 11, T], "ints/record1"))
    return out


def floats():
    shapes = {name: (claim, rows) for name, claim, rows in fold_shapes()}
    out = []
    for pattern, what, extra in (("mixed", "mixed magnitudes", {"teeth": True}), ("-0.0", "every value -0.0", {"sum_bits": 1 << 63}),
                                 ("-0.0/+0.0 last", "-0.0 and +0.0 in the last row", {"last_sum_bits": 0, "sum_bits": 1 << 63})):
        for name in (CUT, THREE):
            claim, rows = shapes[name]
            out.append(_c("%s, %s" % (name, what), dict(claim, **extra), rows, pattern))
    return out


def four_levels():
    """for the device alone: the model does not run 4 M rows, the expectation is integer arithmetic on digits()"""
    return [_c("four levels", {"levels": 4}, [ROWS_PER_FOLD2_TILE - 3, T + 7], "digits")]


def digits(n):
    """the single-digit integers of four_levels, as a numpy array"""
    import numpy as np
    i = np.arange(n, dtype=np.int64)
    return (i * 7 + i // 11) % 19 - 9


def texts(case):
    """the JSON text of every row"""
    return _texts(case.rows, case.pattern)


@functools.lru_cache(maxsize=4)
def _texts(rows, pattern):
    n = sum(rows)
    kind, _, bad = pattern.partition("/")
    if kind == "ints":  # small integers of both signs: every float sum is exact in any association
        out = [str((i + 1) * (-1 if i % 3 == 2 else 1)) for i in range(n)]
        if bad == "11":
            out = ['"x"' if i % 11 == 10 else t for i, t in enumerate(out)]
        elif bad.startswith("tile"):
            k = int(bad[4:])
            out[k * T:(k + 1) * T] = ['"x"'] * T
        elif bad.startswith("record"):
            k = int(bad[6:])
            a = sum(rows[:k])
            out[a:a + rows[k]] = ["null"] * rows[k]
        return out
    if kind == "mixed":  # normal doubles of magnitude 1e-3 .. 1e12, written so that they parse back exactly
        rnd = random.Random(SEED)
        return [repr(rnd.choice((-1.0, 1.0)) * 10.0 ** rnd.uniform(-3, 12)) for _ in range(n)]
    if kind == "-0.0":
        return ["-0.0"] * (n - 1) + ["0.0" if bad else "-0.0"]
    if kind == "digits":
        return [str(int(x)) for x in digits(n)]
    raise ValueError(pattern)


def doc(case):
    """the NDJSON document: {"v":[rows]} per record for select_rows((b"v",)); own: {"v":row} per record, no selection"""
    tx, at, lines = texts(case), 0, []
    for k in case.rows:
        lines.append('{"v":%s}' % tx[at] if case.own else '{"v":[%s]}' % ",".join(tx[at:at + k]))
        at += k
    return "\n".join(lines).encode()


def offsets(case):
    out = [0]
    for k in case.rows:
        out.append(out[-1] + k)
    return out


def column(case, kind):
    """(value bits, statuses) of the rows' texts, as column_walk.convert gives them for these texts"""
    vals, sts = [], []
    for t in texts(case):
        if t[0] == '"':
            st, x = CW.COL_TYPE, 0
        elif t == "null":
            st, x = CW.COL_NULL, 0
        elif "." in t or "e" in t:  # a float
            d = float(t)
            if kind == FLOAT:
                st, x = CW.COL_OK, CW.f2bits(d)
            elif kind == UINT and d < 0.0:
                st, x = CW.COL_RANGE, 0
            else:
                st, x = CW.COL_OK, int(d) & U64
        else:
            i = int(t)
            if kind == FLOAT:
                st, x = CW.COL_OK, CW.f2bits(float(i))
            elif kind == UINT and i < 0:
                st, x = CW.COL_RANGE, 0
            else:
                st, x = CW.COL_OK, i & U64
        vals.append(x)
        sts.append(st)
    return vals, sts


def holds(case, trace, arrays=None):
    """every entry of the case's claim, read from the trace of its per-record run (own: of its total); -> the claims checked"""
    claim, offs = case.claim, offsets(case)
    n = offs[-1]
    items = trace.items
    seen = []
    for what, want in claim.items():
        if what == "levels":
            assert len(levels(n)) == want == len(trace.tiles), (case.name, what)
        elif what == "tiles":
            assert levels(n) == want, (case.name, what, levels(n))
        elif what == "own":
            assert case.own and set(case.rows) == {1}
        elif what == "stored":
            for rec, lv in want.items():
                assert trace.stored.get(rec) == lv, (case.name, what, rec, trace.stored.get(rec), lv)
        elif what == "cut":
            assert offs[1] == want
        elif what == "b_at_255":  # a B item that is the last item of a tile of level 1
            assert any(slot == "B" and (2 * b + 1) % T == T - 1 for b, slot, fl in items[0]), (case.name, what)
        elif what == "a_end_first_slot":  # an A item with END that is the first item of a tile of level 1 behind the first
            assert any(slot == "A" and fl & END and b and (2 * b) % T == 0 for b, slot, fl in items[0]), (case.name, what)
        elif what == "a_open_first_slot":
            assert any(slot == "A" and not fl & END and b and (2 * b) % T == 0 for b, slot, fl in items[0]), (case.name, what)
        elif what == "a_open_whole_tile":  # level 1: a tile whose slot A is VALID and not END and that has no B
            hit = [b for b, slot, fl in items[1] if slot == "A" and fl == VALID and (b, "B", VALID | HEAD) not in items[1]]
            assert hit == [want], (case.name, what, items[1])
            lo = want * (T // 2)  # every row tile below it: slot A open, slot B empty
            below = [(b, slot, fl) for b, slot, fl in items[0] if lo <= b < lo + T // 2]
            assert below == [(b, "A", VALID) for b in range(lo, lo + T // 2)], (case.name, what)
        elif what == "b_from_invalid_last":  # tile 0 of level 1 hands on a B although its last item, slot B of row tile 127, is empty
            assert (0, "B", VALID | HEAD) in items[1] and not any(b == T // 2 - 1 and slot == "B" for b, slot, fl in items[0])
        elif what == "second_fold_ab":
            assert {slot for b, slot, fl in items[1]} == {"A", "B"} and len(trace.tiles) == 3, (case.name, what)
        elif what == "head_in_wave":  # record 1: its first row in that wave of its row tile, its B item in that wave of its fold tile
            b = offs[1] // T
            assert offs[1] % T // 64 == want and (b, "B", VALID | HEAD) in items[0] and (2 * b + 1) % T // 64 == want, (case.name, what)
            assert (offs[2] - 1) // T - b > T // 8 and 2 * ((offs[2] - 1) // T) // T == 2 * b // T  # ... and it ends two waves on
        elif what == "empty_at":
            assert tuple(sorted({a for a, b in zip(offs[:-1], offs[1:]) if a == b})) == want, (case.name, what)
            if arrays is not None:
                assert all(col[r] == 0 for col in arrays for r, (a, b) in enumerate(zip(offs[:-1], offs[1:])) if a == b)
        elif what == "heads_at":
            assert set(want) <= set(offs) and F - 1 in want and F in want
        elif what == "all_at_level":
            assert set(trace.stored.values()) == {want} and len(trace.stored) == n, (case.name, what)
        elif what == "no_items":
            assert all(p == [] for p in items), (case.name, what)
        elif what == "bad_tile":
            sts = column(case, INT)[1]
            assert all(st != CW.COL_OK for st in sts[want * T:(want + 1) * T]) and sts[want * T - 1] == sts[(want + 1) * T] == CW.COL_OK
            assert offs[1] < want * T and offs[2] > (want + 1) * T
        elif what == "all_zero":
            assert case.rows[want] > 2 * T
            if arrays is not None:
                assert arrays[1][want] == case.rows[want] and all(col[want] == 0 for j, col in enumerate(arrays) if j != 1), (case.name, what)
        elif what in ("teeth", "sum_bits", "last_sum_bits"):
            continue  # (the float claims: tests/test_agg_geometry.py::test_float_cases_have_teeth)
        else:
            raise KeyError(what)
        seen.append(what)
    return seen
