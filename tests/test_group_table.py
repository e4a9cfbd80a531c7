"""CPU: the instrument of the key-table tests (tests/group_table.py) against the code the kernels run (csrc/sj_group.h through
sj_selftest_group_* of csrc/host_selftest.cpp): the Python hash is the library's at every key length and pointer alignment, the
byte compare sees a difference in every byte, the capacity is a power of two of at least 64 and twice the rows; every constructor
gives what it promises under the LIBRARY's hash; and every seam family shows its stated property in the serial model for the
forward, the reverse and three shuffled insertion orders -- the device inserts concurrently, so only such properties count."""
import ctypes as C
import os
import random
import re

import pytest

import __graft_entry__ as G
import group_table as GT

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "simdjson-go_amd", "csrc")
U64 = (1 << 64) - 1
FAMILIES = GT.families()


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(G.build_selftest())
    L.sj_selftest_group_hash_bytes.argtypes, L.sj_selftest_group_hash_bytes.restype = [C.c_void_p, C.c_uint64], C.c_uint64
    L.sj_selftest_group_hash_int.argtypes, L.sj_selftest_group_hash_int.restype = [C.c_uint64], C.c_uint64
    L.sj_selftest_group_bytes_equal.argtypes, L.sj_selftest_group_bytes_equal.restype = [C.c_void_p, C.c_void_p, C.c_uint64], C.c_int
    L.sj_selftest_group_table_capacity.argtypes, L.sj_selftest_group_table_capacity.restype = [C.c_uint64], C.c_uint64
    return L


def at_alignment(data, align):
    """a buffer that holds `data` at an address = align mod 8 (kept alive by the caller), and that address"""
    buf = C.create_string_buffer(len(data) + 16)
    base = C.addressof(buf)
    at = base + (align - base) % 8
    C.memmove(at, bytes(data), len(data))
    return buf, at


def lib_hash(lib, key, align=0):
    if isinstance(key, int):
        return lib.sj_selftest_group_hash_int(key & U64)
    buf, at = at_alignment(key, align)
    return lib.sj_selftest_group_hash_bytes(at, len(key))


# ---- the constants come from the headers -----------------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    group_h = open(os.path.join(CSRC, "sj_group.h")).read()
    query = open(os.path.join(CSRC, "query.hip")).read()
    assert re.search(r"static constexpr u64 COL_SHORT = (\d+);", query).group(1) == str(GT.COL_SHORT)
    assert "wide = len > COL_SHORT;" in query[query.index("void k_q_group_emit"):query.index("void k_q_group_bounds")]
    assert re.search(r"u64 cap = (\d+);", group_h).group(1) == str(GT.MIN_CAPACITY)
    assert re.search(r"static constexpr u32 GROUP_NONE = 0x([0-9a-f]+)u;", group_h).group(1) == "%x" % GT.GROUP_NONE
    assert group_h.count("k + 8 <= len; k += 8") == 2 and GT.WORD == 8  # the hash and the compare step by the same word
    for c in (GT.C1, GT.C2, GT.GOLD, GT.RMUL):
        assert "0x%xull" % c in group_h
    assert "blockIdx.x * 256 + threadIdx.x" in query[query.index("void k_q_group_insert"):query.index("void k_q_group_first")] and GT.BLOCK == 256


# ---- the hash --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", list(range(26)) + [31, 32, 33])
def test_hash_bytes_every_length_and_alignment(lib, length):
    rnd = random.Random(length)
    for data in (bytes(rnd.randrange(256) for _ in range(length)), bytes([0xFF]) * length, bytes(length), GT.ALPHABET[:length]):
        want = GT.hash_bytes(data)
        assert [lib_hash(lib, data, a) for a in range(8)] == [want] * 8, (length, data)


def test_hash_int(lib):
    rnd = random.Random(7)
    for x in [0, 1, -1, -(1 << 63), (1 << 63) - 1] + [rnd.randrange(-(1 << 63), 1 << 63) for _ in range(500)]:
        assert lib_hash(lib, x) == GT.hash_int(x), x
        assert GT.unhash_int(GT.hash_int(x)) == x


def test_hash_bytes_random_keys(lib):
    rnd = random.Random(11)
    for _ in range(500):
        data = bytes(rnd.randrange(256) for _ in range(rnd.randrange(200)))
        assert lib_hash(lib, data, rnd.randrange(8)) == GT.hash_bytes(data), data


def test_inverses():
    rnd = random.Random(13)
    for _ in range(500):
        h, w = rnd.getrandbits(64), rnd.getrandbits(64)
        assert GT.unmix(GT.mix(h)) == h == GT.mix(GT.unmix(h))
        assert GT.unround(h, GT.word_round(h, w)) == w and GT.word_round(h, GT.unround(h, w)) == w


# ---- the byte compare ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 7, 8, 9, 16, 17, 24])
def test_bytes_equal_sees_every_byte(lib, length):
    a = bytes((37 * i + 5) % 251 for i in range(length))
    for align_a, align_b in ((0, 0), (1, 5), (7, 2)):
        buf_a, pa = at_alignment(a, align_a)
        buf_same, ps = at_alignment(a, align_b)
        assert lib.sj_selftest_group_bytes_equal(pa, ps, length) == 1
        for j in range(length):
            for flip in (0x01, 0x80):
                b = a[:j] + bytes([a[j] ^ flip]) + a[j + 1:]
                buf_b, pb = at_alignment(b, align_b)
                assert lib.sj_selftest_group_bytes_equal(pa, pb, length) == 0, (length, j, flip)
                assert lib.sj_selftest_group_bytes_equal(pb, pa, length) == 0, (length, j, flip)
    assert lib.sj_selftest_group_bytes_equal(pa, pa, 0) == 1  # no byte differs


# ---- the capacity ----------------------------------------------------------------------------------------------------------------------
def test_capacity(lib):
    ns = [0, 1, 31, 32, 33, 64, 65] + [1 << k for k in range(1, 33)] + [(1 << k) + 1 for k in range(1, 33)]
    for n in ns:
        cap = lib.sj_selftest_group_table_capacity(n)
        assert cap == GT.capacity(n) and cap & (cap - 1) == 0 and cap >= 64 and cap >= 2 * n, n
        assert cap == 64 or cap < 4 * n, n  # and the smallest such
    assert [GT.capacity(n) for n in (32, 33, 64, 65, 600)] == [64, 128, 128, 256, 2048]


# ---- the constructors, under the library's hash ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot,mask,k", [(63, 63, 32), (40, 63, 32), (127, 127, 11), (21, 127, 11), (85, 127, 11), (2047, 2047, 6), (2040, 2047, 300), (0, 63, 5)])
def test_keys_at_a_slot(lib, slot, mask, k):
    ints = GT.int_keys_at(slot, mask, k)
    assert len(set(ints)) == k and all(-(1 << 63) <= x < 1 << 63 and lib_hash(lib, x) & mask == slot for x in ints)
    strs = GT.string_keys_at(slot, mask, k, 16)
    assert len(set(strs)) == k and all(len(s) == 16 and lib_hash(lib, s, 3) & mask == slot for s in strs)
    assert all(b in GT.ALPHABET for s in strs for b in s)
    odd = GT.string_keys_at(slot, mask, min(k, 4), 21)
    assert all(len(s) == 21 and lib_hash(lib, s) & mask == slot for s in odd)


def test_int_keys_with_chosen_hashes(lib):
    hashes = [0, 1, U64, 1 << 63, 0x40, 0x123456789ABCDEF0]
    assert [lib_hash(lib, x) for x in GT.int_keys_with(hashes)] == hashes


@pytest.mark.parametrize("length,same", [(16, False), (19, False), (24, True), (24, False), (35, True)])
def test_colliding_strings(lib, length, same):
    keys = GT.colliding_strings(4, length, same)
    assert len(set(keys)) == 4 and all(len(s) == length for s in keys)
    assert len({lib_hash(lib, s, a) for a, s in enumerate(keys)}) == 1
    assert all(b in GT.ALPHABET for s in keys for b in s) and b'"' not in GT.ALPHABET and b"\\" not in GT.ALPHABET
    assert len({s[length - length % 8:] for s in keys}) == 1  # the tail is shared
    words = [[s[j:j + 8] for j in range(0, length - length % 8, 8)] for s in keys]
    if same:  # equal up to the last two words, which both differ: a compare that stops after an equal word calls them equal
        for a in range(4):
            for b in range(a):
                assert words[a][:-2] == words[b][:-2] and words[a][-2] != words[b][-2] and words[a][-1] != words[b][-1]
    for a in range(4):
        for b in range(a):
            buf_a, pa = at_alignment(keys[a], 1)
            buf_b, pb = at_alignment(keys[b], 6)
            assert lib.sj_selftest_group_bytes_equal(pa, pb, length) == 0


def test_search_bounds_are_fixed():
    """the candidate counts are written down; a constructor that needs more fails (its own assertion), it does not search on"""
    assert (GT.BATCH, GT.AT_CANDIDATES_PER_KEY, GT.COLLIDE_CANDIDATES) == (1 << 16, 8, 1 << 17)
    with pytest.raises(AssertionError, match="bound exceeded"):
        GT.colliding_strings(4000, 16)  # far more than 2^17 / 3300 hits exist


# ---- the families ----------------------------------------------------------------------------------------------------------------------
def test_the_families_are_the_issue_s():
    want = {"collide16", "collide19", "collide24", "copy_seam"} | {n + k for n in ("home63_", "home40_", "repeats63_", "capacity_step_", "blocks_cycle_", "blocks_chain_")
                                                                   for k in ("int", "str")}
    assert set(FAMILIES) == want and set(GT.WRAP_FAMILIES) <= want
    for name, f in FAMILIES.items():
        assert f.capacity == GT.capacity(f.rows) and (f.rows <= 32) == (f.capacity == 64), name
        assert all(isinstance(k, int) for k in f.keys) if f.kind == "int" else all(k is None or isinstance(k, bytes) for k in f.keys), name
    assert [FAMILIES[n].rows for n in ("collide16", "home63_int", "capacity_step_str", "blocks_cycle_int", "blocks_chain_str")] == [16, 32, 33, 600, 600]
    assert [len(FAMILIES[n].distinct()) for n in ("collide24", "home63_str", "repeats63_int", "capacity_step_int", "blocks_cycle_str", "blocks_chain_int")] == [4, 32, 8, 33, 6, 300]
    seam = FAMILIES["copy_seam"]
    assert sorted({len(k) for k in seam.keys}) == GT.SEAM_LENGTHS and all(seam.keys.count(k) in (1, 2) for k in seam.keys)
    for n in GT.SEAM_LENGTHS:
        twice = [k for k in seam.distinct() if len(k) == n and seam.keys.count(k) == 2]
        twins = [k for k in seam.distinct() if len(k) == n and seam.keys.count(k) == 1]
        assert len(twice) == 1 and (n == 0 or (len(twins) == 1 and twins[0][:-1] == twice[0][:-1] and twins[0][-1] != twice[0][-1])), n


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_family_property_in_every_order(lib, name):
    f = FAMILIES[name]
    for k in f.distinct():  # the model's hash is the library's on these very keys
        assert lib_hash(lib, k, 5) == GT.hash_key(k)
    n = f.rows
    f.check()
    f.check(list(reversed(range(n))), reverse=True)
    for seed in (1, 2, 3):
        order = list(range(n))
        random.Random(seed).shuffle(order)
        f.check(order)
    if name in GT.WRAP_FAMILIES:
        assert f.wraps and f.mask in f.cluster and 0 in f.cluster, name
    if name.startswith("collide"):
        assert len({GT.hash_key(k) for k in f.distinct()}) == 1 and f.false_hits == 6


def test_repeats_have_a_later_row_in_front_of_another_key():
    f = FAMILIES["repeats63_int"]
    first = {k: f.keys.index(k) for k in f.distinct()}
    second = {k: [r for r, x in enumerate(f.keys) if x == k][1] for k in f.distinct()}
    assert sum(any(second[a] < first[b] for b in first) for a in first) >= 6


@pytest.mark.parametrize("name", ["copy_seam", "collide19", "home63_str"])
def test_keys_lie_at_every_alignment_in_the_message(name):
    f = FAMILIES[name]
    doc = ('{"rows":[%s]}' % ",".join(GT.rows_json(f))).encode()
    starts = set()
    at = 0
    for k in f.keys:
        if k is None:
            continue
        at = doc.index(b'"k":"', at) + 5
        assert doc[at:at + len(k)] == k
        starts.add(at % 8)
    assert starts == set(range(8)), starts
