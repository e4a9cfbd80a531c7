"""A row predicate by membership in a set, restated on (Tape, Strings.B, Message) arrays -- the checker of the device calls
sjhip_where_path_in / sjhip_count_where_path_in (test infrastructure, on where_walk.satisfies and rows_walk.RowWalk.find_path).

  EQ_OF          the single predicate behind a kind: COL_STRING -> OP_EQ_STRING, COL_INT -> OP_EQ_INT, COL_UINT -> OP_EQ_UINT
  set_values     the caller's values as the predicate takes them: bytes; the 64 bits of an INT value read as int64, of a UINT value
                 as uint64 (what the C call does with int64_t[] / uint64_t[])
  matches        THE DEFINITION: any(satisfies(row, EQ, s) for s in set) -- one single-predicate test per value
  key_of         the row's key as the EQ operator of the kind converts it (None: nothing usable), so that
                 `key_of(...) in set` is the definition at the cost of one conversion; tests/test_where_in_walk.py pins the two
                 against each other
  where_in       one call: the rows of the selection (None: the records, one row each) whose key is in the set, or with negate
                 exactly the others -> (row_offsets, row_index, statuses), where_walk.where's shape
  table, probe   the device's table over the set (tests/group_table.py model: the values in index order) and the probe of a key
                 through it -> (found, slots looked at, wrapped, equal hashes with other bytes): what a family exercises
  families       the constructed sets and row keys of the GPU test, each with what it must show (asserted on the CPU by
                 tests/test_where_in_walk.py)

Pinned by tests/test_where_in_walk.py."""
import collections
import functools

import column_walk as CW
import group_table as GT
import query_walk as Q
import rows_walk as RW
import where_walk as WW

COL_STRING = 4
EQ_OF = {COL_STRING: Q.OP_EQ_STRING, CW.COL_INT: Q.OP_EQ_INT, CW.COL_UINT: Q.OP_EQ_UINT}
WHERE_IN_MAX_VALUES = 1 << 24
MAX_STRING = 1024
M64 = (1 << 64) - 1


def set_values(kind, values):
    if kind == COL_STRING:
        return [bytes(v) for v in values]
    bits = [int(v) & M64 for v in values]
    return [b - (1 << 64) if b >> 63 else b for b in bits] if kind == CW.COL_INT else bits


def matches(w, v, kind, values):
    return any(WW.satisfies(w, v, EQ_OF[kind], s) for s in values)


def key_of(w, v, kind):
    if kind == COL_STRING:
        return w.string_at(v) if chr(w.t[v] >> 56) == '"' else None
    st, bits = CW.convert(w, v, kind)
    if st != CW.COL_OK:
        return None
    return bits - (1 << 64) if kind == CW.COL_INT and bits >> 63 else bits


def where_in(w, sel, path, kind, values, negate=False, by_definition=False):
    values = set_values(kind, values)
    have = frozenset(values)
    offs, index, sts = WW.records_selection(w) if sel is None else sel
    rw = RW.RowWalk(w, index)
    before, new_index = [0], []  # before[i]: the kept rows in front of row i
    for v0 in rw.rows:
        v = rw.find_path(v0 - 1, list(path)) if len(path) else v0
        ok = v < Q.NOT_OBJECT and (matches(w, v, kind, values) if by_definition else key_of(w, v, kind) in have)
        if bool(ok) != bool(negate):
            new_index.append(v0)
        before.append(len(new_index))
    return [before[o] for o in offs], new_index, list(sts)


# ---- the table over the set ------------------------------------------------------------------------------------------------------------
def table(kind, values):
    """the set's table filled in index order (the device fills it concurrently: what holds for every order is what Family states)"""
    values = set_values(kind, values)
    return GT.model(values, GT.capacity(len(values)) - 1)


Probe = collections.namedtuple("Probe", "found steps wrapped false_hits")


def probe(kind, values, key, filled=None):
    values = set_values(kind, values)
    mask = GT.capacity(len(values)) - 1
    filled = filled or GT.model(values, mask)
    h = GT.hash_key(key)
    s, steps, wrapped, false_hits = h & mask, 0, False, 0
    while True:
        steps += 1
        cur = filled.table.get(s)
        if cur is None:
            return Probe(False, steps, wrapped, false_hits)
        if GT.hash_key(values[cur]) == h:
            if values[cur] == key:
                return Probe(True, steps, wrapped, false_hits)
            false_hits += 1
        if s == mask:
            wrapped = True
        s = (s + 1) & mask


class Family:
    """kind; values: the set; keys: the key of every row (None: the row has no "k"); says; and what the CPU test asserts:
    capacity: the table's slots; chain: the occupied slots, exactly (None: not stated); wraps: the fill crosses the last slot;
    long_miss: a row key NOT in the set whose probe looks at at least this many slots and ends at an empty one; false_hits: a row
    key meets at least this many set values of its own 64-bit hash and other bytes"""

    def __init__(self, kind, values, keys, says, capacity, chain=None, wraps=False, long_miss=0, false_hits=0):
        self.kind, self.values, self.keys, self.says = kind, list(values), list(keys), says
        self.capacity, self.chain, self.wraps, self.long_miss, self.false_hits = capacity, chain, wraps, long_miss, false_hits

    def kept(self):
        have = frozenset(set_values(self.kind, self.values))
        return [k is not None and k in have for k in self.keys]

    def rows_json(self):
        """one NDJSON line per row, an odd-length filler in front of the key (the keys lie at every alignment in the message)"""
        out = []
        for r, k in enumerate(self.keys):
            pad = "p" * (2 * (r % 8) + 1)
            if k is None:
                out.append('{"p":"%s"}' % pad)
            else:
                out.append('{"p":"%s","k":%s}' % (pad, str(k) if self.kind != COL_STRING else '"%s"' % k.decode()))
        return out


def _run(home, count, mask):
    return {(home + j) & mask for j in range(count)}


@functools.lru_cache(maxsize=None)
def families():
    fam = {}
    I, S = CW.COL_INT, COL_STRING

    def home(kind, slot, mask, k, salt=0):
        if kind == I:
            return GT.int_keys_at(slot, mask, k, salt)
        return list(GT.string_keys_at(slot, mask, k, 16, stream=1 + salt))

    for kind, tag in ((I, "int"), (S, "str")):
        # 32 values: 64 slots.  All homed at the last slot: the chain is 63, 0 .. 30.  Row keys: the values; keys homed at 63 and
        # keys homed in the middle of the chain (slot 10) that are not in the set -- their probe ends at the empty slot 31
        both = home(kind, 63, 63, 40)
        vals, strangers = both[:32], both[32:]
        middle = home(kind, 10, 63, 4, salt=3)
        fam["home63_" + tag] = Family(kind, vals, vals[::-1] + strangers + middle + [None],
                                      "32 values homed at the last of 64 slots, strangers homed there and in the middle of the chain",
                                      64, _run(63, 32, 63), True, long_miss=33)
        # 33 values: 128 slots.  All homed at slot 120: the chain crosses 127 -> 0
        both = home(kind, 120, 127, 40)
        vals, strangers = both[:33], both[33:]
        middle = home(kind, 2, 127, 4, salt=5)
        fam["home120_" + tag] = Family(kind, vals, strangers + vals + middle,
                                       "33 values (the capacity step to 128 slots) homed at slot 120: the chain crosses the last slot",
                                       128, _run(120, 33, 127), True, long_miss=34)
    # values with one 64-bit hash; row keys with that hash and other bytes: an equal first word (24), a tail (19)
    for length, same in ((16, False), (19, False), (24, True)):
        keys = list(GT.colliding_strings(4, length, same))
        fam["collide%d" % length] = Family(S, keys[:2], [keys[2], keys[0], keys[3], keys[1], keys[2]],
                                           "two %d-byte values with one 64-bit hash, row keys with that hash and other bytes%s" % (
                                               length, ", equal in the first word" if same else ""), 64, None, False, false_hits=2)
    # a row equal to a value but for its last byte, and but for its length
    base = [bytes(GT.ALPHABET[(5 * j + 3 * i) % 93] for i in range(n)) for j, n in enumerate((1, 7, 8, 9, 17, 33))]
    twins = [b[:-1] + bytes([GT.ALPHABET[(GT.ALPHABET.index(b[-1]) + 1) % 93]]) for b in base]
    shorter, longer = [b[:-1] for b in base], [b + b"!" for b in base]
    fam["twins"] = Family(S, base, base + twins + shorter + longer, "row keys that differ from a value in the last byte only, or in the length only",
                          64)
    return fam
