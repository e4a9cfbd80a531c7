"""CPU: the row schema in the result-lifecycle state of a context (csrc/sj_result.h: the eighth Product, `schema`, with the
transitions drop_schema and publish_schema), replayed by csrc/host_selftest.cpp beside the transitions
tests/test_members_result_state.py covers: the schema is published on a resident or sharded state only, is given up by its own drop
(the first step of sjhip_row_schema behind its argument checks), is dropped by everything that drops the other products, and
touches nothing else -- the selection, its `members` property, the parents, the grouping, the order and every other product stay
exactly as they were, which is what "a discovery call leaves the selection alone" means in this state."""
import pytest

from test_group_result_state import GROUP_CALL, GROUPS
from test_members_result_state import M, MEMBERS_CALL, ORDER_LIMIT_CALL, WHERE_CALL
from test_order_result_state import ORDER, ORDER_CALL
from test_result_state import (BEGIN, CALLS, DONE_EMPTY, DONE_SHARD, DROP, PARSE, PENDING, PENDING_, PRODUCT_BIT, RESIDENT, SHARDED, SHARDED_, W,
                               run)  # noqa: F401  (run: the fixture)
from test_rows_result_state import ROWS, SELECT_RECORDS, SELECT_ROWS
from test_unnest_result_state import PARENTS, UNNEST_CALL

DROP_SCHEMA, PUB_SCHEMA = 37, 38
SCHEMA = 1 << 18
SCHEMA_CALL, FAILED_SCHEMA_CALL = [DROP_SCHEMA, PUB_SCHEMA], [DROP_SCHEMA]


def test_schema_transitions(run):
    for seq, want in [
        (PARSE + SCHEMA_CALL, W | SCHEMA), (PARSE + SCHEMA_CALL + SCHEMA_CALL, W | SCHEMA),
        (PARSE + SCHEMA_CALL + FAILED_SCHEMA_CALL, W),  # a call that fails behind its checks leaves no schema
        (PARSE + SCHEMA_CALL + [], W | SCHEMA),         # ... one that fails in them touches nothing
        ([PUB_SCHEMA], 0), ([PENDING, PUB_SCHEMA], PENDING_), ([DONE_EMPTY, PUB_SCHEMA], 0),  # published on a resident result only
        ([DONE_SHARD, PUB_SCHEMA], RESIDENT | SCHEMA), ([SHARDED, PUB_SCHEMA], SHARDED_ | SCHEMA),
        # dropped by what drops the other products
        (PARSE + SCHEMA_CALL + PARSE, W), (PARSE + SCHEMA_CALL + [BEGIN], 0), (PARSE + SCHEMA_CALL + [DROP], 0),
        (PARSE + SCHEMA_CALL + [PENDING], PENDING_), (PARSE + SCHEMA_CALL + [DONE_EMPTY], 0), (PARSE + SCHEMA_CALL + [SHARDED], SHARDED_),
        # the selection in force is read and left: rows, members, parents stay, whether the call succeeds or fails behind its checks
        (PARSE + SELECT_ROWS + SCHEMA_CALL, W | ROWS | SCHEMA), (PARSE + MEMBERS_CALL + SCHEMA_CALL, M | SCHEMA),
        (PARSE + MEMBERS_CALL + WHERE_CALL + SCHEMA_CALL, M | SCHEMA), (PARSE + MEMBERS_CALL + FAILED_SCHEMA_CALL, M),
        (PARSE + UNNEST_CALL + SCHEMA_CALL, W | ROWS | PARENTS | SCHEMA),
        (PARSE + MEMBERS_CALL + ORDER_LIMIT_CALL + GROUP_CALL + SCHEMA_CALL, M | ORDER | GROUPS | SCHEMA),
        # ... and it stays when the selection changes or goes
        (PARSE + SELECT_ROWS + SCHEMA_CALL + SELECT_RECORDS, W | SCHEMA), (PARSE + SCHEMA_CALL + MEMBERS_CALL, M | SCHEMA),
        (PARSE + SCHEMA_CALL + UNNEST_CALL + ORDER_CALL + GROUP_CALL, W | ROWS | PARENTS | ORDER | GROUPS | SCHEMA),
    ]:
        assert run(seq)[-1] == want, (seq, want)


@pytest.mark.parametrize("call", ["filter", "serialize", "marshal", "column", "list_numbers", "list_strings", "query"])
def test_schema_survives_and_is_survived(run, call):
    bit = PRODUCT_BIT.get(call, 0)
    assert run(PARSE + SCHEMA_CALL + CALLS[call])[-1] == W | SCHEMA | bit
    assert run(PARSE + CALLS[call] + SCHEMA_CALL)[-1] == W | SCHEMA | bit
    assert run(PARSE + CALLS[call] + SCHEMA_CALL + FAILED_SCHEMA_CALL)[-1] == W | bit
    assert run(PARSE + MEMBERS_CALL + CALLS[call] + SCHEMA_CALL)[-1] == M | SCHEMA | bit


@pytest.mark.parametrize("call", ["parse", "failed_parse", "stage1_only", "trim", "deserialize"])
def test_schema_is_dropped(run, call):
    after = W if call == "parse" else 0
    assert run(PARSE + MEMBERS_CALL + SCHEMA_CALL + CALLS[call])[-1] == after


def test_no_other_transition_touches_the_schema_and_it_touches_nothing_else(run):
    """from every state the closure reaches: only publish_schema sets the bit, only drop_schema and the transitions that drop a
    result clear it, and the two new codes change no other bit; the earlier codes never set it"""
    assert all(b & SCHEMA == 0 for b in run(list(range(37))))
    ops = list(range(39))
    seen, todo = {0: []}, [0]
    while todo:
        s = todo.pop()
        for op in ops:
            bits = run(seen[s] + [op])
            after, before = bits[-1], bits[-2] if len(bits) > 1 else 0
            assert before == s
            if after & SCHEMA and not before & SCHEMA:
                assert op == PUB_SCHEMA and after & (RESIDENT | SHARDED_)
            if before & SCHEMA and not after & SCHEMA:
                assert op == DROP_SCHEMA or op <= SHARDED
            if op in (DROP_SCHEMA, PUB_SCHEMA):
                assert after & ~SCHEMA == before & ~SCHEMA
            if op == DROP_SCHEMA:
                assert after == before & ~SCHEMA
            if op > SHARDED and op not in (DROP_SCHEMA, PUB_SCHEMA):
                assert after & SCHEMA == before & SCHEMA
            if after not in seen:
                seen[after] = seen[s] + [op]
                todo.append(after)
    without = {s & ~SCHEMA for s in seen}
    assert len(seen) == len(without) + sum(1 for s in without if s & (RESIDENT | SHARDED_))  # one more independent bit on every state with a result
