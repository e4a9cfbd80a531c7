"""The key table of the grouping by several keys (csrc/query.hip: k_q_group_keys, k_q_group_insert; the fold of the tuple hash:
csrc/sj_group.h group_tuple_fold) made controllable from outside, on top of tests/group_table.py: the fold in Python and its
inverse in the last column's hash, constructors of tuples with a chosen 64-bit tuple hash or a chosen home slot -- the last column
is INT and solved --, a serial model of the table over tuples, and the seam families built from them.  No GPU import.

  fold / unfold          group_tuple_fold, and the column hash that takes a running hash to a chosen next one
  tuple_hash             the hash of a tuple of entries (bytes, int, or None for "no key"), as the device folds it column by column:
                         the first entry's hash begins it, so a tuple of one entry hashes as group_table.hash_key of that entry
  solve_last_int         the int64 last entry that gives a prefix of entries a chosen tuple hash
  model                  group_table.model over tuples (equality is the tuple's, entry by entry)
  families               name -> Family: colliding tuples with ONE 64-bit tuple hash, tuples homed at one slot of a 64-slot table whose
                         chain crosses the last slot, repeats in three blocks, and tuples of 8 columns equal on every column but one
  rows_json              the rows of a family as JSON objects with the members c0, c1, ...
The model is an instrument (does a family reach the seam it names, in every order?); the verdict of the GPU tests is
group_multi_walk.group alone.  Pinned, with the fold, by tests/test_group_multi_table.py."""
import functools

import group_table as GT

M64 = GT.M64
NO_KEY_HASH, TMUL = 0x6A09E667F3BCC909, GT.RMUL


def fold(acc, h):
    return GT.mix((acc * TMUL + h) & M64)


def unfold(acc, after):
    """the column hash h with fold(acc, h) == after"""
    return (GT.unmix(after) - acc * TMUL) & M64


def entry_hash(e):
    return NO_KEY_HASH if e is None else GT.hash_key(e)


def tuple_hash(entries):
    """(an empty tuple has no hash: None)"""
    acc = None
    for e in entries:
        acc = entry_hash(e) if acc is None else fold(acc, entry_hash(e))
    return acc


def solve_last_int(prefix, target):
    x = GT.unhash_int(unfold(tuple_hash(prefix), target) if prefix else target)  # (no prefix: the column's hash is the tuple's)
    assert tuple_hash(tuple(prefix) + (x,)) == target and -(1 << 63) <= x < 1 << 63
    return x


def model(tuples, mask, order=None):
    """k_q_group_insert with the rows inserted one after another in `order`; tuples[r] None: a row in no group.  -> group_table.Filled"""
    n = len(tuples)
    hashes = [None if t is None else tuple_hash(t) for t in tuples]
    assert sum(t is not None for t in tuples) <= mask
    table, slot, probe = {}, [None] * n, [None] * n
    wrapped, false_hits, lowered = False, 0, set()
    for r in (range(n) if order is None else order):
        if tuples[r] is None:
            continue
        s, steps = hashes[r] & mask, 0
        while True:
            cur = table.get(s)
            if cur is None:
                table[s] = r
                break
            if hashes[cur] == hashes[r]:
                if tuples[cur] == tuples[r]:
                    if cur > r:
                        table[s] = r
                        if steps:
                            lowered.add(s)
                    break
                false_hits += 1
            if s == mask:
                wrapped = True
            s, steps = (s + 1) & mask, steps + 1
        slot[r], probe[r] = s, steps
    return GT.Filled(slot, probe, wrapped, false_hits, lowered, table)


class Family(GT.Family):
    """group_table.Family over tuples: keys[r] is the tuple of row r (an entry None: the row has no member for that column)"""

    def __init__(self, kinds, keys, says, cluster, max_probe, wraps, false_hits=0, lowered=0):
        GT.Family.__init__(self, "tuple", keys, says, cluster, max_probe, wraps, false_hits, lowered)
        self.kinds = kinds  # "s" / "i" per column

    def check(self, order=None, reverse=False):
        m = model(self.keys, self.mask, order)
        assert set(m.table) == self.cluster, (self.says, sorted(m.table))
        assert self.max_probe is None or max(p for p in m.probe if p is not None) == self.max_probe, self.says
        assert m.wrapped == self.wraps and m.false_hits >= self.false_hits, (self.says, m.wrapped, m.false_hits)
        first = {}
        for r, k in enumerate(self.keys):
            first.setdefault(k, r)
        assert sorted(m.table.values()) == sorted(first.values()), self.says  # every tuple ends as its first row, in one slot
        assert all(m.table[m.slot[r]] == first[k] for r, k in enumerate(self.keys)), self.says
        if reverse:
            assert len(m.lowered_probed) >= self.lowered, (self.says, m.lowered_probed)
        return m


def tuples_with(prefixes, hashes):
    """the prefixes, each closed by the int64 that gives it its hash of `hashes`"""
    out = [tuple(p) + (solve_last_int(p, h),) for p, h in zip(prefixes, hashes)]
    assert [tuple_hash(t) for t in out] == list(hashes) and len(set(out)) == len(out)
    return out


def tuples_at(slot, mask, k, salt=0):
    """k distinct (string, int) tuples whose tuple hash & mask == slot; the bits above the mask are those of a mix"""
    hashes = [(GT.mix((salt << 32) + i + 1) & ~mask & M64) | slot for i in range(k)]
    return tuples_with([(b"make-%d" % (i % 5),) for i in range(k)], hashes)


@functools.lru_cache(maxsize=None)
def families():
    fam = {}
    one = 0x0123456789ABCDEF
    four = tuples_with([(b"alpha",), (b"beta",), (b"gamma-gamma-gamma",), (b"",)], [one] * 4)
    h = one & 63
    fam["collide"] = Family("si", [four[j] for j in GT.COLLIDE_PATTERN if j is not None],
                            "four different (string, int) tuples with one 64-bit tuple hash: only the entries tell them apart",
                            GT._run(h, 4, 63), 3, h + 3 > 63, false_hits=6, lowered=3)
    fam["home40"] = Family("si", tuples_at(40, 63, 32), "32 distinct tuples homed at slot 40 of 64: the chain crosses 63 -> 0",
                           GT._run(40, 32, 63), 31, True)
    fam["capacity_step"] = Family("si", tuples_at(127, 127, 33, salt=1), "33 rows, 128 slots: a chain of 33 from the last slot",
                                  GT._run(127, 33, 127), 32, True)
    six = four + tuples_with([(b"delta",), (b"epsilon",)], [one] * 2)
    f = fam["blocks_collide"] = Family("si", [six[r % 6] for r in range(600)],
                                       "600 rows in three blocks, 6 tuples with one tuple hash cycling: every slot probed for and lowered",
                                       GT._run(one & 2047, 6, 2047), 5, False, false_hits=15, lowered=5)
    assert f.capacity == 2048 and one & 2047 < 2040
    homed = tuples_at(2047, 2047, 6, salt=2)
    fam["blocks_cycle"] = Family("si", [homed[r % 6] for r in range(600)],
                                 "600 rows in three blocks, 6 tuples homed at slot 2047 of 2048 cycling: the chain wraps",
                                 GT._run(2047, 6, 2047), 5, True, lowered=5)
    # 8 columns: a base tuple and, for each position, its twin that differs there only -- a string position and an int position alike
    base = tuple(b"col%d" % c if c % 2 == 0 else 100 + c for c in range(8))
    twins = [base] + [base[:p] + ((base[p] + b"x",) if p % 2 == 0 else (base[p] + 1,)) + base[p + 1:] for p in range(8)]
    rows = twins + twins[::-1]
    occupied = set(model(rows, GT.capacity(len(rows)) - 1).table)
    fam["all_but_one"] = Family("sisisisi", rows, "9 tuples of 8 columns, equal on every column but one, for each position of that one, twice",
                                occupied, None, False)
    return fam


def rows_json(fam):
    """the rows as JSON texts: members c0, c1, ... (strings of the printable alphabet, or integers) and the value v"""
    out = []
    for r, t in enumerate(fam.keys):
        members = ['"c%d":%s' % (c, ('"%s"' % e.decode()) if isinstance(e, bytes) else str(e)) for c, e in enumerate(t)]
        out.append("{%s,\"v\":%d}" % (",".join(members), GT.value_of(r)))
    return out


def key_columns(fam, S, I):
    return [((b"c%d" % c,), S if k == "s" else I) for c, k in enumerate(fam.kinds)]
