"""The open-addressing key table of the grouping (csrc/query.hip: k_q_group_keys, k_q_group_insert, k_q_group_first, k_q_group_emit;
hash, key equality and capacity: csrc/sj_group.h) made controllable from outside: the hash in Python, its inverses, constructors of
keys with a chosen home slot or a chosen full hash, a serial model of the table that says what a set of rows exercises, and the
seam documents built from them.  No GPU import.

"The result of the grouping does not depend on the hash" (sj_group.h) -- so natural keys leave the table's behaviour to chance:
a 64-bit hash never repeats between different keys, a table of at least twice the rows is mostly empty, and a chain reaches the
last slot only by luck.  Everything here is constructed instead:

  mix / unmix              group_mix and its inverse (odd multiplies and xor-shifts are bijections of 64 bits)
  word_round / unround     the per-word round of group_hash_bytes, and the word that takes a state to a chosen next state
  hash_int / unhash_int    group_hash_int and the int64 key of a chosen hash
  hash_bytes               group_hash_bytes
  capacity                 group_table_capacity
  int_keys_with            int64 keys with the given hashes                        (inversion)
  int_keys_at              k distinct int64 keys whose home slot under `mask` is `slot`   (inversion)
  string_keys_at           the same for printable keys of a given length              (counted search)
  colliding_strings        k distinct printable keys with EQUAL 64-bit hashes        (counted search over one word, the last solved)
  model                    the table filled serially in a given row order: slot and probe length per row, the wrap, the
                           comparisons of equal hashes with different keys, the slots lowered after they were reached by probing
  families                 the seam documents: name -> Family (key kind, the key of every row, what it exercises, what the model
                           must show for EVERY insertion order -- the device inserts concurrently)
  rows_json                the rows of a family as the elements of {"rows":[...]}: an odd-length filler in front of the key, so
                           the keys lie at every alignment in the message; a small integer value

The searches are counted, not timed: candidate i of a stream is the i-th number written in the 93 printable bytes that need no
escape, and the number of candidates is written below.  A constructor that does not find what it was asked for raises.

The model is an instrument (does a family reach the seam it names, in every order?); the verdict of the GPU tests is
group_walk.group alone.  WORD, COL_SHORT and MIN_CAPACITY come from csrc/sj_group.h and csrc/query.hip and are pinned, with the
hash, by tests/test_group_table.py."""
import collections
import functools

import numpy as np

M64 = (1 << 64) - 1
C1, C2 = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53  # group_mix
GOLD = 0x9E3779B97F4A7C15
RMUL = 0x9FB21C651E98DF25  # the word round
INV_C1, INV_C2, INV_RMUL = (pow(c, -1, 1 << 64) for c in (C1, C2, RMUL))
WORD = 8  # bytes hashed and compared per step
COL_SHORT = 32  # query.hip: a key of up to COL_SHORT bytes is copied by its lane, a longer one by the wave
MIN_CAPACITY = 64
BLOCK = 256  # rows per block of the per-row kernels
GROUP_NONE = 0xFFFFFFFF

ALPHABET = bytes(b for b in range(0x20, 0x7F) if b not in b'"\\')  # printable, spelled in JSON as itself
assert len(ALPHABET) == 93
_ALPHA = np.frombuffer(ALPHABET, dtype=np.uint8)
_IS_ALPHA = np.zeros(256, dtype=bool)
_IS_ALPHA[_ALPHA] = True

# the candidate counts of the searches (conditions, not measurements: tests/test_group_table.py fails when one is exceeded)
BATCH = 1 << 16
AT_CANDIDATES_PER_KEY = 8   # string_keys_at tries at most this many times (mask + 1) candidates per key asked for
COLLIDE_CANDIDATES = 1 << 17  # colliding_strings: a solved word is printable with probability (93/256)^8 = 1/3300


# ---- the hash ------------------------------------------------------------------------------------------------------------------------
def mix(h):
    h ^= h >> 33
    h = h * C1 & M64
    h ^= h >> 33
    h = h * C2 & M64
    return h ^ h >> 33


def unmix(h):
    h ^= h >> 33  # (a shift of more than half the width undoes itself)
    h = h * INV_C2 & M64
    h ^= h >> 33
    h = h * INV_C1 & M64
    return h ^ h >> 33


def word_round(h, w):
    h = (h ^ mix(w)) * RMUL & M64
    return h ^ h >> 29


def unround(h, after):
    """the word w with word_round(h, w) == after"""
    x = after ^ after >> 29 ^ after >> 58
    return unmix(x * INV_RMUL & M64 ^ h)


def hash_int(x):
    return mix(x & M64 ^ GOLD)


def unhash_int(h):
    x = unmix(h) ^ GOLD
    return x - (1 << 64) if x >> 63 else x


def hash_bytes(s):
    s = bytes(s)
    h = GOLD ^ (len(s) * C1 & M64)
    k = 0
    while k + WORD <= len(s):
        h = word_round(h, int.from_bytes(s[k:k + WORD], "little"))
        k += WORD
    return mix(h ^ int.from_bytes(s[k:], "little"))


def hash_key(key):
    return hash_int(key) if isinstance(key, int) else hash_bytes(key)


def capacity(n):
    cap = MIN_CAPACITY
    while cap < 2 * n:
        cap <<= 1
    return cap


# the same on arrays of uint64 (array arithmetic wraps)
_U = np.uint64


def _mix_np(h):
    h = np.atleast_1d(h)  # (a numpy scalar would warn where an array wraps)
    h = h ^ h >> _U(33)
    h = h * _U(C1)
    h = h ^ h >> _U(33)
    h = h * _U(C2)
    return h ^ h >> _U(33)


def _unmix_np(h):
    h = np.atleast_1d(h)
    h = h ^ h >> _U(33)
    h = h * _U(INV_C2)
    h = h ^ h >> _U(33)
    h = h * _U(INV_C1)
    return h ^ h >> _U(33)


def _round_np(h, w):
    h = (h ^ _mix_np(w)) * _U(RMUL)
    return h ^ h >> _U(29)


def _unround_np(h, after):
    after = np.atleast_1d(after)
    x = after ^ after >> _U(29) ^ after >> _U(58)
    return _unmix_np(x * _U(INV_RMUL) ^ h)


def _candidate_words(stream, first, count):
    """candidates first .. first + count of a stream as 8-byte words: the number stream * 2^40 + i written in base 93, digit d as
    ALPHABET[d], low digit in the low byte.  Different numbers give different words (2^48 < 93^8)"""
    assert 0 <= stream < 256 and first + count <= 1 << 40
    c = (np.arange(first, first + count, dtype=np.uint64) + _U(stream << 40))
    out = np.zeros(count, dtype=np.uint64)
    for j in range(WORD):
        out |= _ALPHA[(c % _U(93)).astype(np.int64)].astype(np.uint64) << _U(8 * j)
        c //= _U(93)
    return out


def _word_bytes(w):
    return int(w).to_bytes(WORD, "little")


def _printable_words(w):
    return _IS_ALPHA[np.ascontiguousarray(w).view(np.uint8).reshape(-1, WORD)].all(axis=1)


# ---- constructors --------------------------------------------------------------------------------------------------------------------
def int_keys_with(hashes):
    keys = [unhash_int(h) for h in hashes]
    assert [hash_int(k) for k in keys] == list(hashes) and all(-(1 << 63) <= k < 1 << 63 for k in keys)
    return keys


def int_keys_at(slot, mask, k, salt=0):
    """k distinct int64 keys with hash & mask == slot; the bits above the mask are those of mix(salt, i), so nothing else about the
    hashes is regular"""
    assert mask & (mask + 1) == 0 and 0 <= slot <= mask
    hashes = [(mix((salt << 32) + i + 1) & ~mask & M64) | slot for i in range(k)]
    keys = int_keys_with(hashes)
    assert len(set(keys)) == k and all(hash_int(x) & mask == slot for x in keys)
    return keys


_BODY = b"bcdfghjklmnpqrstvwxz" * 8


@functools.lru_cache(maxsize=None)
def string_keys_at(slot, mask, k, length, stream=1):
    """k distinct printable keys of `length` >= 8 bytes with hash & mask == slot: the first word is the candidate, the rest is fixed"""
    assert mask & (mask + 1) == 0 and 0 <= slot <= mask and WORD <= length <= len(_BODY)
    rest = _BODY[:length - WORD]
    words = [int.from_bytes(rest[j:j + WORD], "little") for j in range(0, len(rest) - WORD + 1, WORD)]
    tail = int.from_bytes(rest[len(words) * WORD:], "little")
    h0 = _U(GOLD ^ (length * C1 & M64))
    limit, found, first = AT_CANDIDATES_PER_KEY * (mask + 1) * k, [], 0
    while len(found) < k and first < limit:
        cand = _candidate_words(stream, first, min(BATCH, limit - first))
        h = _round_np(h0, cand)
        for w in words:
            h = _round_np(h, _U(w))
        h = _mix_np(h ^ _U(tail))
        found += [_word_bytes(w) + rest for w in cand[(h & _U(mask)) == _U(slot)]]
        first += BATCH
    found = tuple(found[:k])
    assert len(found) == k, ("string_keys_at: bound exceeded", slot, mask, k, length, limit)
    assert len(set(found)) == k and all(len(s) == length and hash_bytes(s) & mask == slot for s in found)
    return found


@functools.lru_cache(maxsize=None)
def colliding_strings(k, length, same_first_word=False, stream=2):
    """k distinct printable keys of `length` bytes with equal 64-bit hashes.  The words in front of the last two are fixed (and so
    shared) with same_first_word, else they follow the candidate; the word before the last is the candidate; the last word is the
    one that takes the candidate's state to the state of candidate 0 -- kept when it is printable; the tail is shared"""
    nw, nt = length // WORD, length % WORD
    assert nw >= (3 if same_first_word else 2)
    tail = _BODY[:nt]
    cand = _candidate_words(stream, 0, COLLIDE_CANDIDATES)
    lead = []
    for j in range(nw - 2):
        lead.append(np.full(COLLIDE_CANDIDATES, int.from_bytes(b"GROUPKEY", "little"), dtype=np.uint64) if same_first_word
                    else _candidate_words(stream + 1 + j, 0, COLLIDE_CANDIDATES))
    h = np.full(COLLIDE_CANDIDATES, GOLD ^ (length * C1 & M64), dtype=np.uint64)
    for w in lead + [cand]:
        h = _round_np(h, w)
    target = _round_np(h[:1], _U(int.from_bytes(b"01234567", "little")))[0]  # candidate 0 ends in this word
    last = _unround_np(h, target)
    hits = np.flatnonzero(_printable_words(last))[:k]
    assert len(hits) == k, ("colliding_strings: bound exceeded", k, length, same_first_word, COLLIDE_CANDIDATES)
    keys = tuple(b"".join(_word_bytes(w[i]) for w in lead + [cand, last]) + tail for i in hits)
    assert len(set(keys)) == k and len({hash_bytes(s) for s in keys}) == 1 and all(len(s) == length for s in keys)
    assert all(b in ALPHABET for s in keys for b in s)
    if same_first_word:
        assert len({s[:WORD * (nw - 2)] for s in keys}) == 1 and len({s[WORD * (nw - 2):WORD * (nw - 1)] for s in keys}) == k
        assert len({s[WORD * (nw - 1):WORD * nw] for s in keys}) == k
    return keys


# ---- the serial model ----------------------------------------------------------------------------------------------------------------
Filled = collections.namedtuple("Filled", "slot probe wrapped false_hits lowered_probed table")


def model(keys, mask, order=None):
    """k_q_group_insert with the rows inserted one after another in `order` (default: row order); keys[r] None: a row without a key.
    slot[r] / probe[r]: where row r ended and after how many steps (None without a key); wrapped: a probe stepped from slot `mask` to
    slot 0; false_hits: comparisons that met an equal hash and a different key; lowered_probed: slots reached after at least one step
    whose occupant was lowered to a smaller row; table: slot -> row"""
    n = len(keys)
    hashes = [None if k is None else hash_key(k) for k in keys]
    assert sum(k is not None for k in keys) <= mask  # an empty slot always exists
    table, slot, probe = {}, [None] * n, [None] * n
    wrapped, false_hits, lowered = False, 0, set()
    for r in (range(n) if order is None else order):
        if keys[r] is None:
            continue
        s, steps = hashes[r] & mask, 0
        while True:
            cur = table.get(s)
            if cur is None:
                table[s] = r
                break
            if hashes[cur] == hashes[r]:
                if keys[cur] == keys[r]:
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
    return Filled(slot, probe, wrapped, false_hits, lowered, table)


# ---- the seam documents --------------------------------------------------------------------------------------------------------------
class Family:
    """kind: "int" / "str"; keys: the key of every row (None: the row has no "k"); says: what it exercises; expect: what the model
    shows for every insertion order --
        cluster      the occupied slots, exactly
        max_probe    the longest probe of any row (None: not stated)
        wraps        whether a probe crosses mask -> 0
        false_hits   at least this many comparisons of equal hashes with different keys
    and, for the reverse row order only (the larger row of every key claims first), lowered: at least this many slots reached by
    probing are lowered to a smaller row"""

    def __init__(self, kind, keys, says, cluster, max_probe, wraps, false_hits=0, lowered=0):
        self.kind, self.keys, self.says = kind, list(keys), says
        self.rows = len(self.keys)
        self.capacity = capacity(self.rows)
        self.mask = self.capacity - 1
        self.cluster, self.max_probe, self.wraps, self.false_hits, self.lowered = set(cluster), max_probe, wraps, false_hits, lowered

    def distinct(self):
        return list(dict.fromkeys(k for k in self.keys if k is not None))

    def check(self, order=None, reverse=False):
        m = model(self.keys, self.mask, order)
        assert set(m.table) == self.cluster, (self.says, sorted(m.table))
        assert self.max_probe is None or max(p for p in m.probe if p is not None) == self.max_probe, self.says
        assert m.wrapped == self.wraps and m.false_hits >= self.false_hits, (self.says, m.wrapped, m.false_hits)
        first = {}
        for r, k in enumerate(self.keys):
            if k is not None:
                first.setdefault(k, r)
        assert sorted(m.table.values()) == sorted(first.values()), self.says  # every key ends as its first row, in one slot
        assert all(m.table[m.slot[r]] == first[k] for r, k in enumerate(self.keys) if k is not None), self.says
        if reverse:
            assert len(m.lowered_probed) >= self.lowered, (self.says, m.lowered_probed)
        return m


def _run(home, count, mask):
    return {(home + j) & mask for j in range(count)}


COLLIDE_PATTERN = [0, 1, 0, None, 2, 1, 3, None, 2, 0, 3, 1, None, 3, 2, 0]  # A B A - C B D - C A D B - D C A
REPEAT_PATTERN = [0, 1, 0, 2, 1, 3, 2, 4, 3, 5, 4, 6, 5, 7, 6, 7, 7, 5, 6, 3, 4, 1, 2, 0, 0, 2, 1, 4, 3, 6, 5, 7]
SEAM_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129]


def _seam_keys():
    """every length twice, and behind the pair a twin that differs in the last byte only"""
    keys = []
    for j, n in enumerate(SEAM_LENGTHS):
        key = bytes(ALPHABET[(7 * j + 3 * i) % 93] for i in range(n))
        keys += [key, key]
        if n:
            keys.append(key[:-1] + bytes([ALPHABET[(ALPHABET.index(key[-1]) + 1) % 93]]))
    return keys[::2] + keys[1::2]  # (the two rows of a key apart)


@functools.lru_cache(maxsize=None)
def families():
    fam = {}

    def home(kind, slot, mask, k, length=16):
        return int_keys_at(slot, mask, k) if kind == "int" else list(string_keys_at(slot, mask, k, length))

    for length, same in ((16, False), (19, False), (24, True)):
        keys = colliding_strings(4, length, same)
        h = hash_bytes(keys[0]) & 63
        fam["collide%d" % length] = Family(
            "str", [None if j is None else keys[j] for j in COLLIDE_PATTERN],
            "four %d-byte keys with one 64-bit hash%s: only the byte compare tells them apart" % (length, ", equal in their first word" if same else ""),
            _run(h, 4, 63), 3, h + 3 > 63, false_hits=6, lowered=3)
    for kind in ("int", "str"):
        assert capacity(32) == 64 and capacity(33) == 128 and capacity(600) == 2048
        fam["home63_" + kind] = Family(kind, home(kind, 63, 63, 32), "32 distinct keys homed at the last of 64 slots: a chain of 32 that wraps at once",
                                       _run(63, 32, 63), 31, True)
        fam["home40_" + kind] = Family(kind, home(kind, 40, 63, 32), "32 distinct keys homed at slot 40 of 64: the chain crosses 63 -> 0",
                                       _run(40, 32, 63), 31, True)
        eight = home(kind, 63, 63, 8)
        assert len(REPEAT_PATTERN) == 32 and all(REPEAT_PATTERN.count(j) == 4 for j in range(8))
        fam["repeats63_" + kind] = Family(kind, [eight[j] for j in REPEAT_PATTERN],
                                          "8 keys x 4 rows homed at slot 63 of 64, later rows of a key in front of other keys' first rows",
                                          _run(63, 8, 63), 7, True, lowered=7)
        # 33 rows: 128 slots.  11 keys at the last slot; 11 + 11 whose hashes agree in the low 6 bits and differ in bit 6
        step = home(kind, 127, 127, 11) + [k for pair in zip(home(kind, 21, 127, 11), home(kind, 85, 127, 11)) for k in pair]
        f = fam["capacity_step_" + kind] = Family(kind, step, "33 rows, 128 slots: a chain from slot 127, and two chains that are one chain under the mask of 32 rows",
                                                  _run(127, 11, 127) | _run(21, 11, 127) | _run(85, 11, 127), 10, True)
        assert f.capacity == 128 and set(model(step[11:], 63).table) == _run(21, 22, 63)
        six = home(kind, 2047, 2047, 6)
        f = fam["blocks_cycle_" + kind] = Family(kind, [six[r % 6] for r in range(600)],
                                                 "600 rows in three blocks, 6 keys homed at slot 2047 of 2048 cycling: every slot of the cluster probed for and lowered",
                                                 _run(2047, 6, 2047), 5, True, lowered=5)
        assert f.capacity == 2048 and all({r // BLOCK for r in range(600) if r % 6 == j} == {0, 1, 2} for j in range(6))
        many = home(kind, 2040, 2047, 300)
        fam["blocks_chain_" + kind] = Family(kind, [many[r % 300] for r in range(600)],
                                             "600 rows, 300 keys homed at slot 2040 of 2048: a chain of 300 across the end", _run(2040, 300, 2047), 299, True,
                                             lowered=299)
    seam = _seam_keys()
    occupied = set(model(seam, capacity(len(seam)) - 1).table)
    fam["copy_seam"] = Family("str", seam, "keys of every length around the 8-byte word and COL_SHORT, twice, and twins that differ in the last byte",
                              occupied, None, False)  # (natural hashes: the longest probe depends on the order)
    assert {WORD - 1, WORD, WORD + 1, 2 * WORD - 1, 2 * WORD, 2 * WORD + 1, COL_SHORT - 1, COL_SHORT, COL_SHORT + 1, 2 * COL_SHORT, 4 * COL_SHORT + 1} <= set(SEAM_LENGTHS)
    return fam


WRAP_FAMILIES = [n + k for n in ("home63_", "capacity_step_", "blocks_cycle_", "blocks_chain_") for k in ("int", "str")]


def value_of(r):
    """the value column: small integers of both signs, every aggregate exact"""
    return (r % 7 + 1) * (-1 if r % 3 == 2 else 1)


def rows_json(fam):
    """the rows as JSON texts.  The filler in front of the key is 1, 3, 5 ... 15 bytes long, so in the message the keys begin at every
    residue of 8 (tests/test_group_table.py); a row without a key has no "k\""""
    out = []
    for r, k in enumerate(fam.keys):
        pad = "p" * (2 * (r % 8) + 1)
        if k is None:
            out.append('{"p":"%s","v":%d}' % (pad, value_of(r)))
        else:
            out.append('{"p":"%s","k":%s,"v":%d}' % (pad, str(k) if fam.kind == "int" else '"%s"' % k.decode(), value_of(r)))
    return out
