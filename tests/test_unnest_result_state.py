"""CPU: the row parents in the result-lifecycle state of a context (csrc/sj_result.h: the seventh Product, `parents`), replayed by
csrc/host_selftest.cpp beside the transitions tests/test_order_result_state.py covers: the product is published on a resident or
sharded state only, is given up by its own begin (the first step of sjhip_unnest_rows behind its argument checks), is dropped by
everything that drops the other products, survives the selection, the order, the grouping, the table, every other product and the
tenants of the shared arenas, and they survive it."""
import pytest

from test_group_result_state import BEGIN_GROUPS, GROUP_CALL, GROUPS, PUB_GROUPS
from test_order_result_state import BEGIN_ORDER, ORDER, ORDER_CALL, PUB_ORDER, PUB_ROWS
from test_result_state import (BEGIN, BEGIN_COL, BEGIN_LIST, CALLS, CLAIM, DONE_EMPTY, DONE_SHARD, DROP, PARSE, PENDING, PENDING_, PRODUCT_BIT,
                               PUB_COL, RESIDENT, SHARDED, SHARDED_, W, run)  # noqa: F401  (run: the fixture)
from test_rows_result_state import BEGIN_ROWS, BEGIN_TABLE, ROWS, SELECT_RECORDS, SELECT_ROWS, TABLE_, TABLE_CALL

BEGIN_PARENTS, PUB_PARENTS = 33, 34
PARENTS = 1 << 16
# sjhip_unnest_rows: its own begin, the new selection published over the old one, the parents published; a call that fails behind
# its checks gives the selection up as well
UNNEST_CALL, FAILED_UNNEST_CALL = [BEGIN_PARENTS, PUB_ROWS, PUB_PARENTS], [BEGIN_PARENTS, BEGIN_ROWS, BEGIN_PARENTS]


def test_parents_transitions(run):
    for seq, want in [
        (PARSE + UNNEST_CALL, W | ROWS | PARENTS), (PARSE + SELECT_ROWS + UNNEST_CALL + UNNEST_CALL, W | ROWS | PARENTS),
        (PARSE + UNNEST_CALL + FAILED_UNNEST_CALL, W),  # a call that fails behind its checks leaves no parents and no selection
        (PARSE + UNNEST_CALL + [], W | ROWS | PARENTS),  # ... one that fails in them touches nothing
        ([PUB_PARENTS], 0), ([PENDING, PUB_PARENTS], PENDING_), ([DONE_EMPTY, PUB_PARENTS], 0),  # published on a resident result only
        ([DONE_SHARD, PUB_PARENTS], RESIDENT | PARENTS), ([SHARDED, PUB_PARENTS], SHARDED_ | PARENTS),
        # dropped by what drops the other products
        (PARSE + UNNEST_CALL + PARSE, W), (PARSE + UNNEST_CALL + [BEGIN], 0), (PARSE + UNNEST_CALL + [DROP], 0),
        (PARSE + UNNEST_CALL + [PENDING], PENDING_), (PARSE + UNNEST_CALL + [DONE_EMPTY], 0), (PARSE + UNNEST_CALL + [SHARDED], SHARDED_),
        ([SHARDED, PUB_PARENTS, PUB_ORDER, PUB_GROUPS, PUB_COL, CLAIM, BEGIN_COL, BEGIN_LIST, BEGIN_TABLE, BEGIN_ROWS, BEGIN_GROUPS, BEGIN_ORDER,
          BEGIN_PARENTS], SHARDED_),
        # untouched by rows.begin(), by a new selection and by a narrowing, and the other way round
        (PARSE + UNNEST_CALL + SELECT_RECORDS, W | PARENTS), (PARSE + SELECT_ROWS + UNNEST_CALL + SELECT_ROWS, W | ROWS | PARENTS),
        (PARSE + SELECT_ROWS + UNNEST_CALL + [PUB_ROWS], W | ROWS | PARENTS), (PARSE + UNNEST_CALL + [BEGIN_PARENTS], W | ROWS),
        # ... by the order, the grouping and the table
        (PARSE + UNNEST_CALL + ORDER_CALL + GROUP_CALL + TABLE_CALL, W | ROWS | PARENTS | ORDER | GROUPS | TABLE_),
        (PARSE + ORDER_CALL + GROUP_CALL + TABLE_CALL + UNNEST_CALL, W | ROWS | PARENTS | ORDER | GROUPS | TABLE_),
        (PARSE + UNNEST_CALL + ORDER_CALL + GROUP_CALL + TABLE_CALL + [BEGIN_ORDER, BEGIN_GROUPS, BEGIN_TABLE], W | ROWS | PARENTS),
        (PARSE + ORDER_CALL + GROUP_CALL + TABLE_CALL + UNNEST_CALL + FAILED_UNNEST_CALL, W | ORDER | GROUPS | TABLE_),
    ]:
        assert run(seq)[-1] == want, (seq, want)


@pytest.mark.parametrize("call", ["filter", "serialize", "marshal", "column", "list_numbers", "list_strings", "query"])
def test_parents_survive_and_are_survived(run, call):
    bit = PRODUCT_BIT.get(call, 0)
    assert run(PARSE + UNNEST_CALL + CALLS[call])[-1] == W | ROWS | PARENTS | bit
    assert run(PARSE + CALLS[call] + UNNEST_CALL)[-1] == W | ROWS | PARENTS | bit
    assert run(PARSE + CALLS[call] + UNNEST_CALL + FAILED_UNNEST_CALL)[-1] == W | bit


@pytest.mark.parametrize("call", ["parse", "failed_parse", "stage1_only", "trim", "deserialize"])
def test_parents_are_dropped(run, call):
    after = W if call == "parse" else 0
    assert run(PARSE + SELECT_ROWS + UNNEST_CALL + CALLS[call])[-1] == after


def test_no_other_transition_touches_the_parents(run):
    """from every state the order closure reaches, with and without the parents: only their publish sets the bit, only their begin
    and the transitions that drop a result clear it"""
    ops = list(range(35))
    seen, todo = {0: []}, [0]
    while todo:
        s = todo.pop()
        for op in ops:
            bits = run(seen[s] + [op])
            after, before = bits[-1], bits[-2] if len(bits) > 1 else 0
            assert before == s
            if after & PARENTS and not before & PARENTS:
                assert op == PUB_PARENTS and after & (RESIDENT | SHARDED_)
            if before & PARENTS and not after & PARENTS:
                assert op == BEGIN_PARENTS or op <= SHARDED
            if op == BEGIN_PARENTS:
                assert after == before & ~PARENTS
            if op > SHARDED and op not in (BEGIN_PARENTS, PUB_PARENTS):
                assert after & PARENTS == before & PARENTS
            if after not in seen:
                seen[after] = seen[s] + [op]
                todo.append(after)
    assert len(seen) == 2 + 2 * 2 * 2 * 4 * (96 + 24 + 12)  # one more independent bit on every state with a result
