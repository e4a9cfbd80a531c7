"""CPU: the instruments of tests/group_multi_table.py are right before the GPU tests lean on them: the Python fold of the tuple hash
is the compiled one (csrc/sj_group.h group_tuple_fold through sj_selftest_group_tuple_hash of csrc/host_selftest.cpp), it depends
on the order of the columns, "no key" is an entry of its own, its last step is inverted exactly, and every family reaches the seam
it names in the forward, the reverse and three shuffled insertion orders -- the device inserts concurrently, so only such
properties count."""
import ctypes as C
import random

import pytest

import __graft_entry__ as G
import group_multi_table as MT
import group_table as GT

U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(G.build_selftest())
    L.sj_selftest_group_tuple_hash.argtypes, L.sj_selftest_group_tuple_hash.restype = [C.c_void_p, C.c_void_p, C.c_uint32], C.c_uint64
    return L


def compiled(lib, entries):
    hs = (C.c_uint64 * len(entries))(*[0 if e is None else GT.hash_key(e) for e in entries])
    has = (C.c_uint8 * len(entries))(*[e is not None for e in entries])
    return lib.sj_selftest_group_tuple_hash(hs, has, len(entries))


def test_fold_is_the_compiled_one(lib):
    rnd = random.Random(5)
    for n in range(1, 9):
        for _ in range(20):
            entries = [rnd.choice([None, rnd.randrange(-(1 << 63), 1 << 63), bytes(rnd.randrange(256) for _ in range(rnd.randrange(20)))])
                       for _ in range(n)]
            assert MT.tuple_hash(entries) == compiled(lib, entries), entries
    src = open(G.os.path.join(G.CSRC, "sj_group.h")).read()
    assert "GROUP_TUPLE_SEED" not in src and "GROUP_NO_KEY_HASH = 0x%xull" % MT.NO_KEY_HASH in src


def test_one_column_hashes_as_that_column(lib):
    """the first column begins the fold, so behind group_paths on one column a key's home slot is the one tests/group_table.py
    constructs for group_path: an int, strings around the 8-byte word and beyond the lane's copy, and "no key\""""
    for e in (7, -(1 << 63), b"", b"1234567", b"12345678", b"123456789", b"x" * 33):
        assert MT.tuple_hash((e,)) == GT.hash_key(e) == compiled(lib, [e]), e
    assert MT.tuple_hash((None,)) == MT.NO_KEY_HASH == compiled(lib, [None])


def test_fold_depends_on_order_boundaries_and_no_key(lib):
    assert MT.tuple_hash((b"x", b"y")) != MT.tuple_hash((b"y", b"x"))
    assert MT.tuple_hash((b"ab", b"c")) != MT.tuple_hash((b"a", b"bc"))
    assert MT.tuple_hash((b"", 1)) != MT.tuple_hash((None, 1)) and MT.tuple_hash((1, None)) != MT.tuple_hash((None, 1))
    assert MT.tuple_hash((7,)) == GT.hash_int(7)  # (one column is not folded: its hash is the tuple's)
    assert MT.tuple_hash((7, 7)) != GT.hash_int(7) and MT.tuple_hash((b"", None)) != MT.tuple_hash((b"",))


def test_the_last_int_column_is_solved_exactly(lib):
    rnd = random.Random(6)
    for prefix in ((), (b"Make",), (None,), (b"a", 5, None, b"long " * 9)):
        acc = MT.tuple_hash(prefix)
        for _ in range(50):
            target = rnd.randrange(1 << 64)
            assert acc is None or MT.fold(acc, MT.unfold(acc, target)) == target  # (no prefix: nothing is folded)
            x = MT.solve_last_int(prefix, target)
            assert compiled(lib, list(prefix) + [x]) == target


def test_the_families_are_the_issue_s():
    fam = MT.families()
    assert len({MT.tuple_hash(t) for t in fam["collide"].keys}) == 1 and len(set(fam["collide"].keys)) == 4
    assert len({MT.tuple_hash(t) for t in fam["blocks_collide"].keys}) == 1 and len(set(fam["blocks_collide"].keys)) == 6
    assert {MT.tuple_hash(t) & 63 for t in fam["home40"].keys} == {40} and fam["home40"].capacity == 64 and fam["home40"].rows == 32
    assert fam["capacity_step"].rows == 33 and fam["capacity_step"].capacity == 128
    assert fam["blocks_cycle"].rows == fam["blocks_collide"].rows == 600 and fam["blocks_cycle"].capacity == 2048
    twins = fam["all_but_one"].keys[:9]
    for p in range(8):  # twin p + 1 differs from the base at column p, and nowhere else
        assert [c for c in range(8) if twins[p + 1][c] != twins[0][c]] == [p]


@pytest.mark.parametrize("name", sorted(MT.families()))
def test_family_property_in_every_order(name):
    f = MT.families()[name]
    n = f.rows
    f.check()
    f.check(list(range(n - 1, -1, -1)), reverse=True)
    for seed in (1, 2, 3):
        order = list(range(n))
        random.Random(seed).shuffle(order)
        f.check(order)
