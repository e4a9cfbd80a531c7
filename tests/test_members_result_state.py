"""CPU: `members` of the row selection in the result-lifecycle state of a context (csrc/sj_result.h ResultState::Rows::members,
the predicate member_rows()), replayed by csrc/host_selftest.cpp: sjhip_unnest_members sets it, every narrowing -- the row
predicates and the limit of an order, which publish through where_narrow -- hands it on, sjhip_select_rows and sjhip_unnest_rows
publish it false, sjhip_select_records and everything that drops a result clear it, and no other product touches it."""
import pytest

from test_group_result_state import GROUP_CALL, GROUPS
from test_order_result_state import ORDER, ORDER_CALL, PUB_ORDER, PUB_ROWS
from test_result_state import CALLS, DONE_SHARD, PARSE, PENDING, PENDING_, PRODUCT_BIT, RESIDENT, SHARDED, SHARDED_, W, run  # noqa: F401
from test_rows_result_state import BEGIN_ROWS, ROWS, SELECT_RECORDS, SELECT_ROWS
from test_unnest_result_state import BEGIN_PARENTS, FAILED_UNNEST_CALL, PARENTS, PUB_PARENTS, UNNEST_CALL

PUB_MEMBER_ROWS, PUB_NARROWED = 35, 36
MEMBERS = 1 << 17
# sjhip_unnest_members: the unnest's transitions with the member selection published; a narrowing (sjhip_where_path[s],
# sjhip_where_row_names) publishes what it kept; an order with a limit narrows, then publishes itself
MEMBERS_CALL = [BEGIN_PARENTS, PUB_MEMBER_ROWS, PUB_PARENTS]
WHERE_CALL = [PUB_NARROWED]
ORDER_LIMIT_CALL = [ORDER_CALL[0], PUB_NARROWED, ORDER_CALL[2]]  # (ORDER_CALL with the narrowing's publish in the place of the plain one)
M = W | ROWS | PARENTS | MEMBERS


def test_members_transitions(run):
    for seq, want in [
        (PARSE + MEMBERS_CALL, M), (PARSE + SELECT_ROWS + MEMBERS_CALL, M), (PARSE + MEMBERS_CALL + MEMBERS_CALL, M),
        # handed on through the narrowings, any number of them
        (PARSE + MEMBERS_CALL + WHERE_CALL, M), (PARSE + MEMBERS_CALL + WHERE_CALL + WHERE_CALL + ORDER_LIMIT_CALL, M | ORDER),
        (PARSE + MEMBERS_CALL + ORDER_LIMIT_CALL, M | ORDER),
        # a narrowing of anything else does not set it: no selection, an array selection, an unnest
        (PARSE + WHERE_CALL, W | ROWS), (PARSE + SELECT_ROWS + WHERE_CALL, W | ROWS), (PARSE + UNNEST_CALL + WHERE_CALL, W | ROWS | PARENTS),
        # cleared by select_rows, unnest_rows, select_records, a failed call, a parse
        (PARSE + MEMBERS_CALL + SELECT_ROWS, W | ROWS | PARENTS), (PARSE + MEMBERS_CALL + UNNEST_CALL, W | ROWS | PARENTS),
        (PARSE + MEMBERS_CALL + WHERE_CALL + UNNEST_CALL + WHERE_CALL, W | ROWS | PARENTS),
        (PARSE + MEMBERS_CALL + SELECT_RECORDS, W | PARENTS), (PARSE + MEMBERS_CALL + SELECT_RECORDS + WHERE_CALL, W | ROWS | PARENTS),
        (PARSE + MEMBERS_CALL + FAILED_UNNEST_CALL, W), (PARSE + MEMBERS_CALL + FAILED_UNNEST_CALL + WHERE_CALL, W | ROWS),
        (PARSE + MEMBERS_CALL + [BEGIN_ROWS], W | PARENTS), (PARSE + MEMBERS_CALL + PARSE, W), (PARSE + MEMBERS_CALL + PARSE + WHERE_CALL, W | ROWS),
        (PARSE + MEMBERS_CALL + [PENDING], PENDING_), (PARSE + MEMBERS_CALL + [SHARDED], SHARDED_),
        # published on a resident or sharded result only
        ([PUB_MEMBER_ROWS], 0), ([PENDING, PUB_MEMBER_ROWS], PENDING_), ([DONE_SHARD, PUB_MEMBER_ROWS], RESIDENT | ROWS | MEMBERS),
        ([SHARDED, PUB_MEMBER_ROWS, PUB_NARROWED], SHARDED_ | ROWS | MEMBERS),
        # the plain publish of the other calls (sjhip_select_rows, sjhip_unnest_rows) is one without members
        (PARSE + MEMBERS_CALL + [PUB_ROWS], W | ROWS | PARENTS),
        # untouched by the parents' own begin, the order and the grouping
        (PARSE + MEMBERS_CALL + [BEGIN_PARENTS], W | ROWS | MEMBERS), (PARSE + MEMBERS_CALL + ORDER_LIMIT_CALL + GROUP_CALL, M | ORDER | GROUPS),
        (PARSE + MEMBERS_CALL + [PUB_ORDER], M | ORDER),
    ]:
        assert run(seq)[-1] == want, (seq, want)


@pytest.mark.parametrize("call", ["filter", "serialize", "marshal", "column", "list_numbers", "list_strings", "query"])
def test_members_survive_the_other_products(run, call):
    bit = PRODUCT_BIT.get(call, 0)
    assert run(PARSE + MEMBERS_CALL + CALLS[call])[-1] == M | bit
    assert run(PARSE + MEMBERS_CALL + CALLS[call] + WHERE_CALL)[-1] == M | bit
    assert run(PARSE + CALLS[call] + MEMBERS_CALL)[-1] == M | bit


@pytest.mark.parametrize("call", ["parse", "failed_parse", "stage1_only", "trim", "deserialize"])
def test_members_are_dropped_with_the_result(run, call):
    after = W if call == "parse" else 0
    assert run(PARSE + MEMBERS_CALL + WHERE_CALL + CALLS[call])[-1] == after


def test_the_earlier_codes_never_set_the_bit(run):
    """what the existing result-state tests observe is unchanged: without the two new codes the bit stays clear, and the new codes
    leave every other bit as the plain publish of the rows does"""
    for seq in (PARSE + SELECT_ROWS + UNNEST_CALL + [PUB_ROWS] + ORDER_CALL + GROUP_CALL, list(range(35)), [SHARDED] + list(range(13, 35))):
        assert all(b & MEMBERS == 0 for b in run(seq))
    for before in (PARSE, PARSE + SELECT_ROWS, PARSE + UNNEST_CALL + ORDER_CALL, [SHARDED], [PENDING], []):
        plain = run(before + [PUB_ROWS])[-1]
        assert run(before + [PUB_MEMBER_ROWS])[-1] == plain | (MEMBERS if plain & ROWS else 0)
        assert run(before + [PUB_NARROWED])[-1] == plain
