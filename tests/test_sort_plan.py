"""CPU: the two pass plans of the device's radix sort (csrc/sj_sort.h) as the selftest library compiles them.  The grouping sorts
codes 0 .. G and takes the low p digits, p the smallest count >= 1 with G < 256^p; the ordering takes the digits in which its keys
differ at all, and agrees with the checker's mirror (tests/order_walk.pass_mask) on the digit sets tests/test_gpu_order.py sorts."""
import ctypes as C
import os
import random

import pytest

import __graft_entry__ as G
import column_walk as CW
import order_walk as OW

DIGIT_SETS = [(d,) for d in range(8)] + [(0, 2), (1, 7), (3, 5)] + [tuple(range(8))]
DIGIT_SETS_LINE = "DIGIT_SETS = [(d,) for d in range(8)] + [(0, 2), (1, 7), (3, 5)] + [tuple(range(8))]\n"
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def plan():
    L = C.CDLL(G.build_selftest())
    L.sj_selftest_sort_plan.argtypes, L.sj_selftest_sort_plan.restype = [C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)], None

    def run(groups, and_, or_):
        out = (C.c_uint32 * 2)()
        L.sj_selftest_sort_plan(groups, and_, or_, out)
        return out[0], out[1]
    return run


@pytest.mark.parametrize("groups", [0, 1, 255, 256, 257, 65535, 65536, (1 << 24) - 1, 1 << 24, 1 << 30])
def test_group_plan_is_the_low_digits(plan, groups):
    p = 1
    while groups >= 256 ** p:
        p += 1
    assert plan(groups, 0, 0)[0] == (1 << p) - 1, (groups, p)


@pytest.mark.parametrize("digits", DIGIT_SETS, ids=lambda ds: "digits-" + "".join(map(str, ds)))
def test_order_plan_agrees_with_the_checker(plan, digits):
    assert DIGIT_SETS_LINE in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_order.py")).read()
    rnd = random.Random(len(digits) * 8 + digits[0])  # (the keys of test_keys_that_differ_in_these_bytes_only)
    base, keys = 0x4142434445464748, []
    for r in range(OW.ORDER_SORT_TILE + 77):
        k = base
        for d in digits:
            k = (k & ~(0xFF << 8 * d)) | (rnd.randrange(256) << 8 * d)
        keys.append(k)
    all_, any_ = U64, 0
    for k in keys:
        all_ &= k
        any_ |= k
    assert plan(0, all_, any_)[1] == OW.pass_mask(keys, [CW.COL_OK] * len(keys), CW.COL_UINT) == sum(1 << d for d in digits)
