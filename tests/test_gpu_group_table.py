"""GPU: the key table of the grouping (csrc/query.hip: k_q_group_keys, k_q_group_insert, k_q_group_first, k_q_group_emit) on the seam
families of tests/group_table.py, whose keys are constructed from the hash (tests/test_group_table.py shows on the CPU that they do
what they say, in every insertion order): different keys with one 64-bit hash, so that only the byte compare tells them apart --
in two words, with a tail, and behind an equal first word; every key homed at one slot, the last of the table or one from which the
chain crosses the end, so that every probe wraps; repeats of keys whose slot is reached by probing and then lowered to the first
row; 33 rows, where the table doubles and a mask from the wrong row count groups wrongly; 600 rows in three blocks on one cluster;
and keys of every length around the 8-byte word and the 32 bytes at which the dictionary copy changes from the lane to the wave.

The verdict is tests/group_walk.group through test_gpu_group.check_group: codes, keys in first-occurrence order, first_row,
group_rows, statuses and the aggregates of a small integer column, all exact; string keys both copied and in the message."""
import numpy as np
import pytest

import column_walk as CW
import group_table as GT
import group_walk as GW
from test_gpu_aggregate import bits
from test_gpu_group import array_rows, check_group
from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

I, S = CW.COL_INT, GW.COL_STRING
FAMILIES = GT.families()
COLLIDE = ["collide16", "collide19", "collide24"]
ONE_SLOT = [n + k for n in ("home63_", "home40_", "repeats63_") for k in ("int", "str")]
STEP = ["capacity_step_int", "capacity_step_str"]
BLOCKS = [n + k for n in ("blocks_cycle_", "blocks_chain_") for k in ("int", "str")]


def cases(names):
    """string keys copied and in the message; INT keys have no bytes: one run"""
    return [pytest.param(n, copy, id="%s-%s" % (n, "copied" if copy else "in-the-message")) for n in names
            for copy in ([True, False] if FAMILIES[n].kind == "str" else [True])]


def run_family(ctx, name, copy=True):
    """the family's rows grouped by "k" with the aggregates of "v": the checker's answer, and what the family is about"""
    f = FAMILIES[name]
    rw = array_rows(ctx, GT.rows_json(f), copy=copy)
    got, want = check_group(ctx, rw, (b"k",), I if f.kind == "int" else S, (b"v",), I, what=(name, copy))
    order = f.distinct()
    assert got.rows == f.rows and got.groups == len(order), name
    assert (got.keys.tolist() if f.kind == "int" else got.keys) == order, name
    assert got.codes.tolist() == [GT.GROUP_NONE if k is None else order.index(k) for k in f.keys], name
    assert got.first_row.tolist() == [f.keys.index(k) for k in order], name
    assert got.sum.tolist() == [sum(GT.value_of(r) for r, x in enumerate(f.keys) if x == k) for k in order], name
    if f.kind == "str":  # the dictionary: every key's bytes at the running sum of the lengths in front
        assert got.key_offsets.dtype == np.uint64 and got.key_offsets.tolist() == np.cumsum([0] + [len(k) for k in order]).tolist(), name
    ctx.select_records()
    return got


@pytest.mark.parametrize("name,copy", cases(COLLIDE))
def test_full_collisions(ctx, name, copy):
    got = run_family(ctx, name, copy)
    assert got.groups == 4 and got.group_rows.tolist() == [GT.COLLIDE_PATTERN.count(j) for j in range(4)]
    assert got.status.tolist().count(CW.COL_NOT_FOUND) == GT.COLLIDE_PATTERN.count(None) == 3


@pytest.mark.parametrize("name,copy", cases(ONE_SLOT))
def test_one_home_slot_of_64(ctx, name, copy):
    got = run_family(ctx, name, copy)
    assert FAMILIES[name].capacity == 64 and got.groups == (8 if name.startswith("repeats") else 32)


@pytest.mark.parametrize("name,copy", cases(STEP))
def test_capacity_step(ctx, name, copy):
    got = run_family(ctx, name, copy)
    assert FAMILIES[name].capacity == 128 and got.groups == 33


@pytest.mark.parametrize("name,copy", cases(BLOCKS))
def test_across_waves_and_blocks(ctx, name, copy):
    got = run_family(ctx, name, copy)
    assert FAMILIES[name].capacity == 2048 and got.rows == 600
    assert got.group_rows.tolist() == ([100] * 6 if "cycle" in name else [2] * 300)


@pytest.mark.parametrize("name", GT.WRAP_FAMILIES + ["collide16"])
def test_the_seams_behind_group_paths_on_one_column(ctx, name):
    """the constructed home slots hold behind the several-keys entry point too (a tuple of one column hashes as that column,
    tests/test_group_multi_table.py): group_paths on the single column "k" against the same verdict, tests/group_walk.group"""
    f = FAMILIES[name]
    kind = I if f.kind == "int" else S
    rw = array_rows(ctx, GT.rows_json(f))
    want = GW.group(rw, (b"k",), kind, (b"v",), I)
    got = ctx.group_paths([((b"k",), kind)], [((b"v",), I)])
    assert (got.rows, got.groups) == (want.rows, want.groups) == (f.rows, len(f.distinct())), name
    assert (got.keys[0] if kind == S else got.keys[0].tolist()) == want.keys == f.distinct(), name
    assert got.key_ok[0].tolist() == [1] * want.groups and got.status[0].tolist() == want.status, name
    assert got.codes.dtype == np.uint32 and got.codes.tolist() == want.codes, name
    assert got.first_row.tolist() == want.first_row and got.group_rows.tolist() == want.group_rows, name
    for j, wanted in enumerate(GW.arrays(want, I)):
        assert np.array_equal(bits(got.values[0][j]), np.array(wanted, dtype=np.uint64)), (name, j)
    ctx.select_records()


@pytest.mark.parametrize("copy", [True, False], ids=["copied", "in-the-message"])
def test_dictionary_copy_seam(ctx, copy):
    got = run_family(ctx, "copy_seam", copy)
    order = FAMILIES["copy_seam"].distinct()
    assert sorted({len(k) for k in got.keys}) == GT.SEAM_LENGTHS and got.key_bytes == sum(map(len, order))
    assert b"".join(got.keys) == b"".join(order)  # no byte too few or too many on either side of COL_SHORT
    assert got.group_rows.tolist() == [FAMILIES["copy_seam"].keys.count(k) for k in order]
