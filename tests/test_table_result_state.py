"""CPU: the table (sjhip_extract_table) in the result-lifecycle state of a context (csrc/sj_result.h), replayed by
csrc/host_selftest.cpp with the op codes appended behind those of tests/test_result_state.py: begin_table, publish_table and the
predicate bit of the table.  The table is dropped by what drops every product, left alone by every other product's transitions
-- and leaves them alone --, and is only published on a result."""
import pytest

import test_result_state as RS
from test_result_state import run  # noqa: F401  (the fixture)

BEGIN_TABLE, PUB_TABLE = 25, 26
TABLE = 1 << 12
W = RS.W


def last(run, seq):
    return run(seq)[-1]


def test_codes_are_appended(run):
    assert max(RS.OPS) == 24 and RS.LIST_STR == 1 << 11
    assert last(run, [RS.DONE_WHOLE, PUB_TABLE]) == W | TABLE
    assert last(run, [RS.DONE_WHOLE, PUB_TABLE, BEGIN_TABLE]) == W


@pytest.mark.parametrize("result, bits", [(RS.DONE_WHOLE, W), (RS.DONE_SHARD, RS.RESIDENT), (RS.SHARDED, RS.SHARDED_)])
def test_dropped_by_what_drops_every_product(run, result, bits):
    have = [result, PUB_TABLE]
    assert last(run, have) == bits | TABLE
    assert last(run, have + [RS.BEGIN]) == 0
    assert last(run, have + [RS.DROP]) == 0
    assert last(run, have + [RS.PENDING]) == RS.PENDING_
    assert last(run, have + [RS.DONE_WHOLE]) == W
    assert last(run, have + [RS.DONE_SHARD]) == RS.RESIDENT
    assert last(run, have + [RS.DONE_EMPTY]) == 0
    assert last(run, have + [RS.SHARDED]) == RS.SHARDED_
    assert last(run, have + [BEGIN_TABLE]) == bits
    assert last(run, have + [BEGIN_TABLE, PUB_TABLE]) == bits | TABLE  # the next sjhip_extract_table


def test_refused_without_a_result(run):
    assert last(run, [PUB_TABLE]) == 0
    assert last(run, [RS.PENDING, PUB_TABLE]) == RS.PENDING_
    assert last(run, [RS.DONE_WHOLE, RS.BEGIN, PUB_TABLE]) == 0
    assert last(run, [RS.DONE_EMPTY, PUB_TABLE]) == 0


def test_independent_of_the_other_products(run):
    """every call of the "call x product" table: the table survives it unless it drops everything, and the call's own product
    and the products it leaves alone are what they are without a table"""
    table_call = [BEGIN_TABLE, PUB_TABLE]
    for call, ops in RS.CALLS.items():
        without = last(run, RS.PARSE + ops)
        got = last(run, RS.PARSE + table_call + ops)
        survives = call not in ("parse", "failed_parse", "stage1_only", "trim", "deserialize")
        assert got == (without | TABLE if survives else without), call
    # ... and the reverse: extract_table touches no other product
    for product, ops in RS.CALLS.items():
        if product not in RS.PRODUCT_BIT:
            continue
        before = last(run, RS.PARSE + ops)
        assert before & RS.PRODUCT_BIT[product]
        assert last(run, RS.PARSE + ops + table_call) == before | TABLE, product
        assert last(run, RS.PARSE + ops + [BEGIN_TABLE]) == before, product
    # every single transition but the parse ones leaves the bit alone
    for op in range(RS.CLAIM, 25):
        assert last(run, [RS.DONE_WHOLE, PUB_TABLE, op]) & TABLE, op
    # a stage-1-only call on the owner of a sharded result: the products go, the shards stay
    assert last(run, [RS.SHARDED, PUB_TABLE, RS.PUB_COL, RS.CLAIM, RS.BEGIN_COL, RS.BEGIN_LIST, BEGIN_TABLE]) == RS.SHARDED_
