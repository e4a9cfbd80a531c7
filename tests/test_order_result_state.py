"""CPU: the order in the result-lifecycle state of a context (csrc/sj_result.h: the sixth Product, `order`), replayed by
csrc/host_selftest.cpp beside the transitions tests/test_group_result_state.py covers: the order is published on a resident or
sharded state only, is given up by its own begin (the first step of sjhip_order_path behind its argument checks), is dropped by
everything that drops the other products, survives the selection, every other product and the tenants of the shared arenas, and
they survive it.  And the host-and-device pieces of csrc/sj_order.h and csrc/sj_sort.h as the same selftest library compiles
them: agg_key is monotone in the order of its kind, and order_pass_mask names exactly the digits in which AND and OR differ."""
import ctypes as C
import struct

import pytest

import __graft_entry__ as G
import aggregate_walk as AW
from test_group_result_state import BEGIN_GROUPS, GROUP_CALL, GROUPS, PUB_GROUPS
from test_result_state import (BEGIN, BEGIN_COL, BEGIN_LIST, CALLS, CLAIM, DONE_EMPTY, DONE_SHARD, DROP, PARSE, PENDING, PENDING_, PRODUCT_BIT,
                               PUB_COL, RESIDENT, SHARDED, SHARDED_, W, run)  # noqa: F401  (run: the fixture)
from test_rows_result_state import BEGIN_ROWS, BEGIN_TABLE, ROWS, SELECT_RECORDS, SELECT_ROWS, TABLE_, TABLE_CALL

BEGIN_ORDER, PUB_ORDER, PUB_ROWS = 31, 32, 28
ORDER = 1 << 15
# sjhip_order_path: its own begin, the narrowed selection published, the order published; a call that fails behind its checks gives
# the selection up as well
ORDER_CALL, FAILED_ORDER_CALL = [BEGIN_ORDER, PUB_ROWS, PUB_ORDER], [BEGIN_ORDER, BEGIN_ROWS]


def test_order_transitions(run):
    for seq, want in [
        (PARSE + ORDER_CALL, W | ROWS | ORDER), (PARSE + ORDER_CALL + ORDER_CALL, W | ROWS | ORDER),
        (PARSE + ORDER_CALL + FAILED_ORDER_CALL, W),  # a call that fails behind its checks leaves no order and no selection
        (PARSE + ORDER_CALL + [], W | ROWS | ORDER),  # ... one that fails in them touches nothing
        ([PUB_ORDER], 0), ([PENDING, PUB_ORDER], PENDING_), ([DONE_EMPTY, PUB_ORDER], 0),  # published on a resident result only
        ([DONE_SHARD, PUB_ORDER], RESIDENT | ORDER), ([SHARDED, PUB_ORDER], SHARDED_ | ORDER),
        # dropped by what drops the other products
        (PARSE + ORDER_CALL + PARSE, W), (PARSE + ORDER_CALL + [BEGIN], 0), (PARSE + ORDER_CALL + [DROP], 0),
        (PARSE + ORDER_CALL + [PENDING], PENDING_), (PARSE + ORDER_CALL + [DONE_EMPTY], 0), (PARSE + ORDER_CALL + [SHARDED], SHARDED_),
        ([SHARDED, PUB_ORDER, PUB_GROUPS, PUB_COL, CLAIM, BEGIN_COL, BEGIN_LIST, BEGIN_TABLE, BEGIN_ROWS, BEGIN_GROUPS, BEGIN_ORDER], SHARDED_),
        # untouched by rows.begin() and by a new selection, and the other way round
        (PARSE + ORDER_CALL + SELECT_RECORDS, W | ORDER), (PARSE + SELECT_ROWS + ORDER_CALL + SELECT_ROWS, W | ROWS | ORDER),
        (PARSE + SELECT_ROWS + ORDER_CALL + [BEGIN_ROWS], W | ORDER), (PARSE + ORDER_CALL + [BEGIN_ORDER], W | ROWS),
        (PARSE + ORDER_CALL + GROUP_CALL + TABLE_CALL, W | ROWS | ORDER | GROUPS | TABLE_),
        (PARSE + GROUP_CALL + TABLE_CALL + ORDER_CALL + [BEGIN_GROUPS, BEGIN_TABLE], W | ROWS | ORDER),
        (PARSE + GROUP_CALL + ORDER_CALL + FAILED_ORDER_CALL, W | GROUPS),
    ]:
        assert run(seq)[-1] == want, (seq, want)


@pytest.mark.parametrize("call", ["filter", "serialize", "marshal", "column", "list_numbers", "list_strings", "query"])
def test_order_survives_and_is_survived(run, call):
    bit = PRODUCT_BIT.get(call, 0)
    assert run(PARSE + ORDER_CALL + CALLS[call])[-1] == W | ROWS | ORDER | bit
    assert run(PARSE + CALLS[call] + ORDER_CALL)[-1] == W | ROWS | ORDER | bit
    assert run(PARSE + CALLS[call] + ORDER_CALL + FAILED_ORDER_CALL)[-1] == W | bit


@pytest.mark.parametrize("call", ["parse", "failed_parse", "stage1_only", "trim", "deserialize"])
def test_order_is_dropped(run, call):
    after = W if call == "parse" else 0
    assert run(PARSE + SELECT_ROWS + ORDER_CALL + CALLS[call])[-1] == after


def test_no_other_transition_touches_the_order(run):
    """from every state the group closure reaches, with and without an order: only its publish sets the bit, only its begin and the
    transitions that drop a result clear it"""
    ops = list(range(33))
    seen, todo = {0: []}, [0]
    while todo:
        s = todo.pop()
        for op in ops:
            bits = run(seen[s] + [op])
            after, before = bits[-1], bits[-2] if len(bits) > 1 else 0
            assert before == s
            if after & ORDER and not before & ORDER:
                assert op == PUB_ORDER and after & (RESIDENT | SHARDED_)
            if before & ORDER and not after & ORDER:
                assert op == BEGIN_ORDER or op <= SHARDED
            if op == BEGIN_ORDER:
                assert after == before & ~ORDER
            if op > SHARDED and op not in (BEGIN_ORDER, PUB_ORDER):
                assert after & ORDER == before & ORDER
            if after not in seen:
                seen[after] = seen[s] + [op]
                todo.append(after)
    assert len(seen) == 2 + 2 * 2 * 4 * (96 + 24 + 12)  # one more independent bit on every state with a result


# ---- sj_order.h, sj_sort.h--------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(G.build_selftest())
    for name in ("sj_selftest_agg_key", "sj_selftest_agg_unkey"):
        getattr(L, name).argtypes, getattr(L, name).restype = [C.c_uint64, C.c_int], C.c_uint64
    L.sj_selftest_order_pass_mask.argtypes, L.sj_selftest_order_pass_mask.restype = [C.c_uint64, C.c_uint64], C.c_uint32
    return L


def f2b(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


U64 = (1 << 64) - 1
DBL_MAX, DENORM = 1.7976931348623157e308, 5e-324
ASCENDING = {
    1: [x & U64 for x in (-(1 << 63), -(1 << 63) + 1, -(1 << 32), -1, 0, 1, 255, 256, 1 << 32, (1 << 63) - 1)],  # INT
    2: [0, 1, 255, 256, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, U64 - 1, U64],  # UINT
    0: [f2b(x) for x in (-DBL_MAX, -1e308, -1.0, -2.2250738585072014e-308, -2 * DENORM, -DENORM, -0.0, 0.0, DENORM, 2 * DENORM,
                         2.2250738585072014e-308, 1.0, 1e308, DBL_MAX)],  # FLOAT
}


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_agg_key_is_monotone(lib, kind):
    keys = [lib.sj_selftest_agg_key(b, kind) for b in ASCENDING[kind]]
    assert keys == sorted(keys) and len(set(keys)) == len(keys), [hex(k) for k in keys]
    assert keys == [AW.key(b, kind) for b in ASCENDING[kind]]  # the checker's key is the device's
    assert [lib.sj_selftest_agg_unkey(k, kind) for k in keys] == ASCENDING[kind]
    # the complement reverses the order: what a descending sort compares
    assert [~k & U64 for k in keys] == sorted((~k & U64 for k in keys), reverse=True)


def test_order_pass_mask(lib):
    mask = lib.sj_selftest_order_pass_mask
    base = 0x1122334455667788
    assert mask(base, base) == 0 and mask(0, 0) == 0 and mask(U64, U64) == 0  # nothing varies: no pass
    assert mask(0, U64) == 0xFF                                                # everything varies: all eight
    for d in range(8):
        for bit in (0, 3, 7):  # one varying bit anywhere in digit d
            v = 1 << (8 * d + bit)
            assert mask(base & ~v, base | v) == 1 << d, (d, bit)
        assert mask(base & ~(0xFF << 8 * d), base | (0xFF << 8 * d)) == 1 << d
    for d, e in [(0, 2), (1, 7), (3, 5), (0, 7)]:  # two digits that are no neighbours
        v = 1 << (8 * d) | 0x80 << (8 * e)
        assert mask(base & ~v, base | v) == (1 << d | 1 << e)
    assert mask(0, (1 << 20) - 1) == 0b111  # counts below 2^20: three passes
