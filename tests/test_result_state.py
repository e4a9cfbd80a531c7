"""CPU: the result-lifecycle state of a context (csrc/sj_result.h), replayed by csrc/host_selftest.cpp -- a hand-written table of
call sequences with the predicates the header's contract promises (every row of DESIGN.md's "call x product" table among them),
and the closure of the reachable states with the invariants checked on every state and every transition."""
import ctypes as C

import pytest

import __graft_entry__ as G

# the byte codes of sj_selftest_result_state
BEGIN, DROP, PENDING = 0, 1, 2
DONE_WHOLE, DONE_WHOLE_PACKED, DONE_WHOLE_KF, DONE_WHOLE_KF_PACKED, DONE_SHARD, DONE_SHARD_PACKED, DONE_SHARD_KF, DONE_SHARD_KF_PACKED = range(3, 11)
DONE_EMPTY, SHARDED, CLAIM, PUB_FILTERED, PUB_SERIALIZED, PUB_MARSHALED, BEGIN_COL, PUB_COL, BEGIN_LIST, PUB_LIST_NUM, PUB_LIST_STR = range(11, 22)
REL_FILTERED, REL_SERIALIZED, REL_MARSHALED = 22, 23, 24
OPS = list(range(25))
# ... and its predicate bits
PENDING_, WHOLE, RESIDENT, SHARDED_, KF, PACKED, FILTERED, SERIALIZED, MARSHALED, COLUMN, LIST_NUM, LIST_STR = (1 << k for k in range(12))
TENANTS = FILTERED | SERIALIZED | MARSHALED
PRODUCTS = TENANTS | COLUMN | LIST_NUM | LIST_STR


@pytest.fixture(scope="module")
def run():
    lib = C.CDLL(G.build_selftest())
    lib.sj_selftest_result_state.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32)]
    lib.sj_selftest_result_state.restype = C.c_int

    def run(ops):
        out = (C.c_uint32 * max(len(ops), 1))()
        assert lib.sj_selftest_result_state(bytes(ops), len(ops), out) == 0
        return list(out[:len(ops)])
    return run


# What the library's calls do to the state (the host files, one line each): a parse is begin, pending, begin, done; a product call
# gives up its own product, claims or begins, then publishes; a count / path query touches nothing.
PARSE = [BEGIN, PENDING, BEGIN, DONE_WHOLE]
CALLS = {
    "filter": [CLAIM, PUB_FILTERED], "serialize": [REL_SERIALIZED, REL_MARSHALED, CLAIM, PUB_SERIALIZED],
    "marshal": [REL_MARSHALED, CLAIM, PUB_MARSHALED],
    "column": [BEGIN_COL, PUB_COL], "list_numbers": [BEGIN_LIST, PUB_LIST_NUM], "list_strings": [BEGIN_LIST, PUB_LIST_STR],
    "query": [], "parse": PARSE, "failed_parse": [BEGIN], "stage1_only": [DROP], "trim": [DROP], "deserialize": [DROP],
}
PRODUCT_BIT = {"filter": FILTERED, "serialize": SERIALIZED, "marshal": MARSHALED, "column": COLUMN, "list_numbers": LIST_NUM,
               "list_strings": LIST_STR}
# DESIGN.md, "call x product": the products a call leaves alone (its own product is replaced); every other cell is "dropped"
SURVIVES = {
    "filter": {"column", "list_numbers", "list_strings"}, "serialize": {"column", "list_numbers", "list_strings"},
    "marshal": {"column", "list_numbers", "list_strings"}, "column": {"filter", "serialize", "marshal", "list_numbers", "list_strings"},
    "list_numbers": {"filter", "serialize", "marshal", "column"}, "list_strings": {"filter", "serialize", "marshal", "column"},
    "query": set(PRODUCT_BIT), "parse": set(), "failed_parse": set(), "stage1_only": set(), "trim": set(), "deserialize": set(),
}

W = WHOLE | RESIDENT
TABLE = [  # (sequence, the predicate set after its last step)
    ([BEGIN], 0), ([DROP], 0), ([PENDING], PENDING_), ([PENDING, BEGIN], 0), ([PENDING, DROP], 0),
    ([PENDING, BEGIN, DONE_WHOLE], W), ([DONE_WHOLE_PACKED], W | PACKED), ([DONE_WHOLE_KF], W | KF), ([DONE_WHOLE_KF_PACKED], W | KF | PACKED),
    ([DONE_SHARD], RESIDENT), ([DONE_SHARD_KF], RESIDENT | KF), ([DONE_SHARD_PACKED], RESIDENT), ([DONE_SHARD_KF_PACKED], RESIDENT | KF),
    ([DONE_EMPTY], 0), ([DONE_WHOLE_KF_PACKED, DONE_EMPTY], 0), ([SHARDED], SHARDED_),
    ([DONE_WHOLE_KF_PACKED, PUB_COL, BEGIN], 0), ([DONE_WHOLE_KF_PACKED, PUB_MARSHALED, PUB_COL, PUB_LIST_STR, DROP], 0),
    ([DONE_WHOLE_PACKED, PENDING], PENDING_), ([SHARDED, PUB_MARSHALED, PUB_COL, DONE_WHOLE], W),
    # products need a result to be published on; the filter and the serializer a whole one
    ([PUB_FILTERED], 0), ([PUB_SERIALIZED], 0), ([PUB_MARSHALED], 0), ([PUB_COL], 0), ([PUB_LIST_NUM], 0), ([PUB_LIST_STR], 0),
    ([PENDING, PUB_MARSHALED], PENDING_), ([PENDING, PUB_COL], PENDING_),
    ([DONE_SHARD, PUB_FILTERED], RESIDENT), ([DONE_SHARD, PUB_SERIALIZED], RESIDENT), ([DONE_SHARD, PUB_MARSHALED], RESIDENT | MARSHALED),
    ([SHARDED, PUB_FILTERED], SHARDED_), ([SHARDED, PUB_SERIALIZED], SHARDED_), ([SHARDED, PUB_MARSHALED], SHARDED_ | MARSHALED),
    ([SHARDED, PUB_COL, PUB_LIST_NUM], SHARDED_ | COLUMN | LIST_NUM), ([DONE_SHARD, PUB_COL, PUB_LIST_STR], RESIDENT | COLUMN | LIST_STR),
    # one tenant; a claim without a publish leaves none
    ([DONE_WHOLE, CLAIM, PUB_FILTERED], W | FILTERED), ([DONE_WHOLE, PUB_FILTERED, CLAIM], W),
    ([DONE_WHOLE, PUB_FILTERED, CLAIM, PUB_SERIALIZED], W | SERIALIZED), ([DONE_WHOLE, PUB_SERIALIZED, CLAIM, PUB_MARSHALED], W | MARSHALED),
    ([DONE_WHOLE, PUB_MARSHALED, CLAIM, PUB_FILTERED], W | FILTERED), ([DONE_WHOLE, PUB_MARSHALED, CLAIM], W),
    # a product call that fails its checks has given up its own product and no other: a refused serialize (it also gives up the
    # MarshalJSON text), a refused marshal; a refused filter touches nothing
    ([DONE_WHOLE, PUB_FILTERED, REL_SERIALIZED, REL_MARSHALED], W | FILTERED), ([DONE_WHOLE, PUB_SERIALIZED, REL_SERIALIZED, REL_MARSHALED], W),
    ([DONE_WHOLE, PUB_MARSHALED, REL_SERIALIZED, REL_MARSHALED], W), ([DONE_WHOLE, PUB_FILTERED, REL_MARSHALED], W | FILTERED),
    ([DONE_WHOLE, PUB_SERIALIZED, REL_MARSHALED], W | SERIALIZED), ([DONE_WHOLE, PUB_MARSHALED, REL_MARSHALED], W),
    ([DONE_WHOLE, PUB_MARSHALED, REL_FILTERED], W | MARSHALED), ([SHARDED, PUB_MARSHALED, PUB_COL, REL_SERIALIZED, REL_MARSHALED], SHARDED_ | COLUMN),
    # a stage-1-only call on the owner of a sharded result: the products go, the shards stay
    ([SHARDED, PUB_MARSHALED, PUB_COL, PUB_LIST_NUM, CLAIM, BEGIN_COL, BEGIN_LIST], SHARDED_),
    ([SHARDED, PUB_COL, PUB_LIST_STR, CLAIM, BEGIN_COL, BEGIN_LIST], SHARDED_),
    # the columns: independent of the tenant and of each other; one list column, of one kind
    ([DONE_WHOLE, PUB_COL, CLAIM, PUB_MARSHALED], W | COLUMN | MARSHALED), ([DONE_WHOLE, PUB_COL, BEGIN_COL], W),
    ([DONE_WHOLE, PUB_COL, PUB_LIST_NUM, BEGIN_COL], W | LIST_NUM), ([DONE_WHOLE, PUB_COL, PUB_LIST_NUM, BEGIN_LIST], W | COLUMN),
    ([DONE_WHOLE, PUB_LIST_NUM, BEGIN_LIST, PUB_LIST_STR], W | LIST_STR), ([DONE_WHOLE, PUB_LIST_STR, BEGIN_LIST, PUB_LIST_NUM], W | LIST_NUM),
    ([DONE_WHOLE_KF, PUB_FILTERED, PUB_COL, PUB_LIST_STR], W | KF | FILTERED | COLUMN | LIST_STR),
]
# every row of the "call x product" table: parse, the product, the call -> the product's bit survives or is gone
for call, keeps in SURVIVES.items():
    for product, bit in PRODUCT_BIT.items():
        if call == product:
            continue
        after = {"parse": W, "failed_parse": 0, "stage1_only": 0, "trim": 0, "deserialize": 0}.get(call, W | PRODUCT_BIT.get(call, 0))
        if product in keeps:
            after |= bit
        TABLE.append((PARSE + CALLS[product] + CALLS[call], after))


def test_table(run):
    assert len(TABLE) > 100
    for seq, want in TABLE:
        assert run(seq)[-1] == want, (seq, want)


def step_invariants(before, op, after):
    assert bin(after & TENANTS).count("1") <= 1 and (after & (LIST_NUM | LIST_STR)) != (LIST_NUM | LIST_STR)
    assert bin(after & (PENDING_ | RESIDENT | SHARDED_)).count("1") <= 1 and (not after & WHOLE or after & RESIDENT)
    if not after & (RESIDENT | SHARDED_):  # nothing derived without a resident result
        assert after & ~PENDING_ == 0
    if not after & WHOLE:
        assert after & (FILTERED | SERIALIZED | PACKED) == 0
    if after & SHARDED_:
        assert after & KF == 0
    if op in (BEGIN, DROP, DONE_EMPTY):
        assert after == 0
    if op == PENDING:
        assert after == PENDING_
    if op == CLAIM:
        assert after == before & ~TENANTS  # (never published: no tenant)
    if op in (REL_FILTERED, REL_SERIALIZED, REL_MARSHALED):
        assert after == before & ~{REL_FILTERED: FILTERED, REL_SERIALIZED: SERIALIZED, REL_MARSHALED: MARSHALED}[op]
    if op == BEGIN_COL:
        assert after == before & ~COLUMN
    if op == BEGIN_LIST:
        assert after == before & ~(LIST_NUM | LIST_STR)
    if DONE_WHOLE <= op <= DONE_SHARD_KF_PACKED or op == SHARDED:
        assert after & PRODUCTS == 0  # a new result has no products
    # a product's bit comes with its publish alone, and only the transitions that drop it take it away
    born = {PUB_FILTERED: FILTERED, PUB_SERIALIZED: SERIALIZED, PUB_MARSHALED: MARSHALED, PUB_COL: COLUMN, PUB_LIST_NUM: LIST_NUM,
            PUB_LIST_STR: LIST_STR}
    parse_ops = set(range(BEGIN, SHARDED + 1))
    drops = {FILTERED: parse_ops | {CLAIM, REL_FILTERED, PUB_SERIALIZED, PUB_MARSHALED},
             SERIALIZED: parse_ops | {CLAIM, REL_SERIALIZED, PUB_FILTERED, PUB_MARSHALED},
             MARSHALED: parse_ops | {CLAIM, REL_MARSHALED, PUB_FILTERED, PUB_SERIALIZED}, COLUMN: parse_ops | {BEGIN_COL},
             LIST_NUM: parse_ops | {BEGIN_LIST, PUB_LIST_STR}, LIST_STR: parse_ops | {BEGIN_LIST, PUB_LIST_NUM}}
    for bit in born.values():
        if after & bit and not before & bit:
            assert born.get(op) == bit, (before, op, after)
        if before & bit and not after & bit:
            assert op in drops[bit], (before, op, after)
    for bit in (KF, PACKED):
        if after & bit and not before & bit:
            assert DONE_WHOLE <= op <= DONE_SHARD_KF_PACKED


def test_closure_of_reachable_states(run):
    """Every state is told apart by its predicates (the sizes are payload), so the search runs over predicate sets: from each new
    one, every transition.  The count, from the contract: nothing and pending (2); a whole result with or without key flags, packed
    or not, one of four tenants, a column or none, one of three list states (2 * 2 * 4 * 2 * 3 = 96); a shard, never packed, with the
    MarshalJSON text as its only possible tenant (2 * 2 * 2 * 3 = 24); a sharded result, without key flags of its own (2 * 2 * 3 = 12)."""
    path = {0: []}
    todo = [0]
    while todo:
        s = todo.pop()
        for op in OPS:
            seq = path[s] + [op]
            bits = run(seq)
            before = bits[-2] if len(bits) > 1 else 0
            assert before == s
            step_invariants(before, op, bits[-1])
            if bits[-1] not in path:
                path[bits[-1]] = seq
                todo.append(bits[-1])
    assert len(path) == 2 + 96 + 24 + 12
