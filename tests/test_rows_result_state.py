"""CPU: the row selection in the result-lifecycle state of a context (csrc/sj_result.h: the fourth Product, `rows`), replayed by
csrc/host_selftest.cpp beside the transitions tests/test_result_state.py covers: the selection is published on a resident or
sharded result only, is given up by its own begin (sjhip_select_records, and the first step of sjhip_select_rows), is dropped by
everything that drops the other products, survives every other product and the tenants of the shared arenas, and they survive it."""
import pytest

from test_result_state import (BEGIN, BEGIN_COL, BEGIN_LIST, CALLS, CLAIM, COLUMN, DONE_EMPTY, DONE_SHARD, DONE_WHOLE, DROP, FILTERED, LIST_NUM,
                               LIST_STR, MARSHALED, PARSE, PENDING, PENDING_, PRODUCT_BIT, PUB_COL, PUB_LIST_NUM, PUB_MARSHALED, RESIDENT,
                               SERIALIZED, SHARDED, SHARDED_, W, run)  # noqa: F401  (run: the fixture)

BEGIN_TABLE, PUB_TABLE, BEGIN_ROWS, PUB_ROWS = 25, 26, 27, 28
TABLE_, ROWS = 1 << 12, 1 << 13
SELECT_ROWS, SELECT_RECORDS, TABLE_CALL = [BEGIN_ROWS, PUB_ROWS], [BEGIN_ROWS], [BEGIN_TABLE, PUB_TABLE]


def test_selection_transitions(run):
    for seq, want in [
        (PARSE + SELECT_ROWS, W | ROWS), (PARSE + SELECT_ROWS + SELECT_RECORDS, W), (PARSE + SELECT_RECORDS + SELECT_RECORDS, W),
        ([PUB_ROWS], 0), ([PENDING, PUB_ROWS], PENDING_), ([DONE_EMPTY, PUB_ROWS], 0),  # nothing to select on
        ([DONE_SHARD, PUB_ROWS], RESIDENT | ROWS), ([SHARDED, PUB_ROWS], SHARDED_ | ROWS),
        (PARSE + SELECT_ROWS + SELECT_ROWS, W | ROWS), (PARSE + SELECT_ROWS + [BEGIN_ROWS], W),  # a select_rows that fails after its begin
        # dropped by what drops the other products
        (PARSE + SELECT_ROWS + PARSE, W), (PARSE + SELECT_ROWS + [BEGIN], 0), (PARSE + SELECT_ROWS + [DROP], 0),
        (PARSE + SELECT_ROWS + [PENDING], PENDING_), (PARSE + SELECT_ROWS + [DONE_EMPTY], 0), (PARSE + SELECT_ROWS + [SHARDED], SHARDED_),
        # a stage-1-only call on the owner of a sharded result: claim, then every product's begin (drop_products)
        ([SHARDED, PUB_ROWS, PUB_COL, CLAIM, BEGIN_COL, BEGIN_LIST, BEGIN_TABLE, BEGIN_ROWS], SHARDED_),
        # a table built under a selection stays when the selection goes, and the other way round
        (PARSE + SELECT_ROWS + TABLE_CALL + SELECT_RECORDS, W | TABLE_), (PARSE + SELECT_ROWS + TABLE_CALL + [BEGIN_TABLE], W | ROWS),
        (PARSE + SELECT_ROWS + [PUB_COL, PUB_LIST_NUM] + TABLE_CALL + SELECT_ROWS, W | ROWS | COLUMN | LIST_NUM | TABLE_),
    ]:
        assert run(seq)[-1] == want, (seq, want)


@pytest.mark.parametrize("call", ["filter", "serialize", "marshal", "column", "list_numbers", "list_strings", "query"])
def test_selection_survives_and_is_survived(run, call):
    bit = PRODUCT_BIT.get(call, 0)
    assert run(PARSE + SELECT_ROWS + CALLS[call])[-1] == W | ROWS | bit   # the call under a selection
    assert run(PARSE + CALLS[call] + SELECT_ROWS)[-1] == W | ROWS | bit   # the selection after the call's product
    assert run(PARSE + CALLS[call] + SELECT_ROWS + SELECT_RECORDS)[-1] == W | bit
    assert run(PARSE + SELECT_ROWS + TABLE_CALL + CALLS[call])[-1] == W | ROWS | TABLE_ | bit


@pytest.mark.parametrize("call", ["parse", "failed_parse", "stage1_only", "trim", "deserialize"])
def test_selection_is_dropped(run, call):
    after = W if call == "parse" else 0
    assert run(PARSE + SELECT_ROWS + TABLE_CALL + CALLS[call])[-1] == after


def test_closure_with_the_selection(run):
    """the reachable predicate sets with the table and the selection among the transitions: each of them is one more independent
    bit on every state with a result, so the 96 + 24 + 12 states of tests/test_result_state.py times four, and the two without"""
    ops = list(range(29))
    seen, todo = {0: []}, [0]
    while todo:
        s = todo.pop()
        for op in ops:
            bits = run(seen[s] + [op])
            after, before = bits[-1], bits[-2] if len(bits) > 1 else 0
            assert before == s
            if not after & (RESIDENT | SHARDED_):
                assert after & ~PENDING_ == 0  # nothing derived, the selection included, without a result
            if after & ROWS and not before & ROWS:
                assert op == PUB_ROWS
            if before & ROWS and not after & ROWS:
                assert op == BEGIN_ROWS or op <= SHARDED
            if op == BEGIN_ROWS:
                assert after == before & ~ROWS
            if after not in seen:
                seen[after] = seen[s] + [op]
                todo.append(after)
    assert len(seen) == 2 + 4 * (96 + 24 + 12)
