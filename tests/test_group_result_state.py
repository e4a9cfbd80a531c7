"""CPU: the grouping in the result-lifecycle state of a context (csrc/sj_result.h: the fifth Product, `groups`), replayed by
csrc/host_selftest.cpp beside the transitions tests/test_result_state.py and tests/test_rows_result_state.py cover: the grouping is
published on a resident or sharded state only, is given up by its own begin (the first step of sjhip_group_path behind its argument
checks), is dropped by everything that drops the other products, survives the selection, every other product and the tenants of the
shared arenas, and they survive it."""
import pytest

from test_result_state import (BEGIN, BEGIN_COL, BEGIN_LIST, CALLS, CLAIM, COLUMN, DONE_EMPTY, DONE_SHARD, DROP, LIST_NUM, PARSE, PENDING,
                               PENDING_, PRODUCT_BIT, PUB_COL, PUB_LIST_NUM, RESIDENT, SHARDED, SHARDED_, W, run)  # noqa: F401  (run: the fixture)
from test_rows_result_state import BEGIN_ROWS, BEGIN_TABLE, ROWS, SELECT_RECORDS, SELECT_ROWS, TABLE_, TABLE_CALL

BEGIN_GROUPS, PUB_GROUPS = 29, 30
GROUPS = 1 << 14
GROUP_CALL, FAILED_GROUP_CALL = [BEGIN_GROUPS, PUB_GROUPS], [BEGIN_GROUPS]


def test_group_transitions(run):
    for seq, want in [
        (PARSE + GROUP_CALL, W | GROUPS), (PARSE + GROUP_CALL + GROUP_CALL, W | GROUPS),
        (PARSE + GROUP_CALL + FAILED_GROUP_CALL, W),  # a call that fails behind its checks leaves no grouping
        (PARSE + GROUP_CALL + [], W | GROUPS),        # ... one that fails in them touches nothing
        ([PUB_GROUPS], 0), ([PENDING, PUB_GROUPS], PENDING_), ([DONE_EMPTY, PUB_GROUPS], 0),  # nothing to group
        ([DONE_SHARD, PUB_GROUPS], RESIDENT | GROUPS), ([SHARDED, PUB_GROUPS], SHARDED_ | GROUPS),
        # dropped by what drops the other products
        (PARSE + GROUP_CALL + PARSE, W), (PARSE + GROUP_CALL + [BEGIN], 0), (PARSE + GROUP_CALL + [DROP], 0),
        (PARSE + GROUP_CALL + [PENDING], PENDING_), (PARSE + GROUP_CALL + [DONE_EMPTY], 0), (PARSE + GROUP_CALL + [SHARDED], SHARDED_),
        ([SHARDED, PUB_GROUPS, PUB_COL, CLAIM, BEGIN_COL, BEGIN_LIST, BEGIN_TABLE, BEGIN_ROWS, BEGIN_GROUPS], SHARDED_),
        # built under a selection, it stays when the selection changes or goes, and the other way round
        (PARSE + SELECT_ROWS + GROUP_CALL + SELECT_RECORDS, W | GROUPS), (PARSE + SELECT_ROWS + GROUP_CALL + SELECT_ROWS, W | ROWS | GROUPS),
        (PARSE + SELECT_ROWS + GROUP_CALL + FAILED_GROUP_CALL, W | ROWS),
        (PARSE + SELECT_ROWS + [PUB_COL, PUB_LIST_NUM] + TABLE_CALL + GROUP_CALL, W | ROWS | COLUMN | LIST_NUM | TABLE_ | GROUPS),
        (PARSE + GROUP_CALL + TABLE_CALL + [BEGIN_TABLE], W | GROUPS),
    ]:
        assert run(seq)[-1] == want, (seq, want)


@pytest.mark.parametrize("call", ["filter", "serialize", "marshal", "column", "list_numbers", "list_strings", "query"])
def test_grouping_survives_and_is_survived(run, call):
    bit = PRODUCT_BIT.get(call, 0)
    assert run(PARSE + GROUP_CALL + CALLS[call])[-1] == W | GROUPS | bit
    assert run(PARSE + CALLS[call] + GROUP_CALL)[-1] == W | GROUPS | bit
    assert run(PARSE + CALLS[call] + GROUP_CALL + FAILED_GROUP_CALL)[-1] == W | bit
    assert run(PARSE + SELECT_ROWS + GROUP_CALL + TABLE_CALL + CALLS[call])[-1] == W | ROWS | GROUPS | TABLE_ | bit


@pytest.mark.parametrize("call", ["parse", "failed_parse", "stage1_only", "trim", "deserialize"])
def test_grouping_is_dropped(run, call):
    after = W if call == "parse" else 0
    assert run(PARSE + SELECT_ROWS + GROUP_CALL + CALLS[call])[-1] == after


def test_closure_with_the_grouping(run):
    """the reachable predicate sets with the grouping among the transitions: one more independent bit on every state with a
    result, so the states of tests/test_rows_result_state.py with a result times two, and the two without"""
    ops = list(range(31))
    seen, todo = {0: []}, [0]
    while todo:
        s = todo.pop()
        for op in ops:
            bits = run(seen[s] + [op])
            after, before = bits[-1], bits[-2] if len(bits) > 1 else 0
            assert before == s
            if not after & (RESIDENT | SHARDED_):
                assert after & ~PENDING_ == 0
            if after & GROUPS and not before & GROUPS:
                assert op == PUB_GROUPS
            if before & GROUPS and not after & GROUPS:
                assert op == BEGIN_GROUPS or op <= SHARDED
            if op == BEGIN_GROUPS:
                assert after == before & ~GROUPS
            if op in (BEGIN_ROWS, BEGIN_TABLE, BEGIN_COL, BEGIN_LIST, CLAIM):
                assert after & GROUPS == before & GROUPS
            if after not in seen:
                seen[after] = seen[s] + [op]
                todo.append(after)
    assert len(seen) == 2 + 2 * 4 * (96 + 24 + 12)
