"""GPU: random call chains over the query layer -- one row selection, seven products, three tenants of the shared arenas -- against
the host model of tests/chain_model.py (its lifetime table is taken from csrc/sj_result.h and include/sjhip.h).  Every chain of
chain_model.CHAINS: 16 steps on one parsed document; after every step the call's return values, after every selection call
fetch_rows, at every fetch everything it returns bit for bit (float sums as tests/test_gpu_aggregate.py compares them: as bits where
every partial sum is exact, else within its float_bound), after every refused fetch and every invalid call everything that lives,
and at the end every live product and tenant once more and find_path on the records.  Half of the chains run on a fresh context,
whose arenas grow during the chain, half on the shared one behind larger parses.  A failure names the first step that differed and
prints the lines that replay the chain.  tests/test_chain_model.py holds the list to the conditions that make this mean something."""
import pytest

import chain_model as CM
import fixtures
from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def large(ctx):  # noqa: F811
    """the shared context behind larger parses and larger products: its arenas are large and nothing moves during a chain"""
    doc = fixtures.load("citm_catalog")
    ctx.parse(doc, key_flags=True)
    ctx.select_rows((b"performances",))
    ctx.unnest_rows((b"seatCategories",))
    ctx.extract_table([((b"seatCategoryId",), CM.I), ((b"areas",), CM.SC)])
    ctx.extract_path_strings((b"areas",), cvt=True)
    ctx.extract_path_list((b"areas",), CM.I)
    ctx.group_path((b"seatCategoryId",), CM.I, (b"seatCategoryId",), CM.I)
    ctx.order_path((b"seatCategoryId",), CM.I)
    ctx.marshal_rows(fetch=False)
    ctx.filter_rows(fetch=False)
    ctx.serialize(fetch=False)
    ctx.select_records()
    return ctx


@pytest.mark.parametrize("chain", CM.CHAINS, ids=CM.chain_id)
def test_chain(large, chain):
    if not chain[3]:
        return CM.run_on(large, chain)
    import sjhip
    fresh = sjhip.Context(0)
    try:
        CM.run_on(fresh, chain)
    finally:
        fresh.close()


@pytest.mark.parametrize("chain", CM.CHAINS_M, ids=CM.chain_id)
def test_member_chain(large, chain):
    """chain_model.CHAINS_M: the chains of the extended generator -- the member rows and their `members` flag through every
    narrowing and every selection change, the row names as the string column, the projection as a tenant and beside live
    products, the two readers --, run and compared as test_chain does"""
    if not chain[3]:
        return CM.run_on(large, chain, extended=True)
    import sjhip
    fresh = sjhip.Context(0)
    try:
        CM.run_on(fresh, chain, extended=True)
    finally:
        fresh.close()


# ---- a sharded result -----------------------------------------------------------------------------------------------------------------
SHARDED_CHAIN = [  # eight steps, drawn only from the calls that accept a sharded result
    ("call", "where_path", ((b"k",), 10, 2, {})),                                   # OP_GE_INT: the records with k >= 2
    ("call", "extract_path_strings", ((b"pad",), {"fetch": False})),
    ("call", "unnest_rows", ((b"t",),)),
    ("call", "aggregate_path", ((), CM.I)),
    ("call", "where_paths", ([((), 10, 5), ((), 7, 9000)], bytes([0, 1, CM.AND]))),  # 5 <= the row's own value < 9000
    ("fetch", "column", ()),
    ("call", "select_records", ()),
    ("call", "extract_table", ([((b"k",), CM.I), ((b"pad",), CM.S)], {"fetch": True})),
]


def test_chain_on_a_sharded_result():
    """The setup of tests/test_gpu_order.py test_sharded_result_is_refused -- fixtures.nd_shard_limits and the padded 11 000-record
    document, every record with one more member, the array "t", so that an unnest has rows to find -- and SHARDED_CHAIN on the
    sharded context and on a second one that parsed the document whole: every return value and every fetched array must be equal.
    Read off csrc (what goes through query_parts / result_parts, and what asks no_whole_result or whole_entry):
      accepted on a sharded result: find_path, count_where_path, count_where_paths, project_keys, extract_path, aggregate_path,
        aggregate_path_records, extract_path_strings, extract_path_list, extract_path_list_strings, extract_table, select_rows,
        select_records, where_path, where_paths, unnest_rows, marshal_json and every fetch of their products;
      refused: filter_where, filter_rows, marshal_rows, serialize, group_path, group_paths, order_path, order_path_strings,
        order_paths.
    Between the steps every refused call is issued on the sharded context: each must return SJHIP_ERR_ARG, and the comparison of
    the next step (and of everything that lives, at the end) shows that it changed nothing."""
    import sjhip
    pad = "x" * 230
    doc = "\n".join('{"pad":"%s","k":%d,"t":[%s]}' % (pad, r % 7, ",".join(str(r + j) for j in range(r % 4))) for r in range(11000)).encode()
    assert len(doc) > 5 << 19
    refused = [lambda c: c.filter_where(b"k", b"1"), lambda c: c.filter_rows(fetch=False), lambda c: c.marshal_rows(fetch=False),
               lambda c: c.serialize(fetch=False), lambda c: c.group_path((b"k",), CM.I, fetch=False),
               lambda c: c.group_paths([((b"k",), CM.I)], fetch=False), lambda c: c.order_path((b"k",), CM.I, fetch=False),
               lambda c: c.order_path_strings((b"pad",), fetch=False), lambda c: c.order_paths([((b"k",), CM.I, False)], fetch=False)]
    many, one = sjhip.Context(0), sjhip.Context(0)
    try:
        with fixtures.nd_shard_limits(2 << 20, 1 << 20):
            many.parse(doc, ndjson=True)
        one.parse(doc, ndjson=True)
        with pytest.raises(sjhip.ParseError):
            many.order_path((b"k",), CM.I)
        assert "sharded" in many.last_error()
        info = {}
        for k, (do, name, args) in enumerate(SHARDED_CHAIN):
            if do == "fetch":
                got, want = (CM.device_fetch(c, name, info[name]) for c in (many, one))
                assert CM.differs(got, want) is None, (k, name, CM.differs(got, want))
            else:
                got, want = (CM.device_call(c, name, args) for c in (many, one))
                assert got[0] == want[0], (k, name, got[0], want[0])
                assert (got[3] is None) == (want[3] is None) and (got[3] is None or CM.differs(got[3], want[3]) is None), (k, name)
                if got[1]:
                    info[got[1]] = got[2]
                if name in CM.SELECTION_CALLS and name != "select_records":
                    sizes = (got[0][0], got[0][-1])
                    info["rows"] = sizes
                    assert CM.differs(CM.device_fetch(many, "rows", sizes), CM.device_fetch(one, "rows", sizes)) is None, (k, name)
            for call in refused:
                with pytest.raises(sjhip.ParseError) as e:
                    call(many)
                assert e.value.code == CM.ERR_ARG, (k, many.last_error())
        assert info["parents"][1] > 5000 and info["column"][0] > 7000  # (the chain ran on rows, not on nothing)
        for what in ("column", "parents", "table"):
            assert CM.differs(CM.device_fetch(many, what, info[what]), CM.device_fetch(one, what, info[what])) is None, what
        assert many.find_path(b"k").tolist() == one.find_path(b"k").tolist()
    finally:
        many.close()
        one.close()


SHARDED_MEMBER_CHAIN = [
    ("call", "unnest_members", ((b"m",),)),
    ("call", "where_row_names", (19, b"b", {"negate": True})),                      # OP_PREFIX_STRING: the members not named b...
    ("call", "extract_row_names", ({"fetch": False},)),
    ("call", "where_path", ((), 10, 20, {})),                                       # OP_GE_INT on the member's own value
    ("call", "aggregate_path_records", ((), CM.I)),
    ("fetch", "column", ()),
    ("call", "select_records", ()),
    ("invalid", "extract_row_names", ("not_members", 4, b"a")),
]


def test_member_chain_on_a_sharded_result():
    """test_chain_on_a_sharded_result for the member rows: the same padded 11 000 records with one more member each, a map "m" of
    r % 4 members, and SHARDED_MEMBER_CHAIN on the sharded context and on one that parsed the document whole -- every return value
    and every array must be equal, and the name call behind select_records is refused on both.  Between the steps every call that
    refuses a sharded result is issued on the sharded context, sjhip_marshal_rows_paths among them (sjhip.h: "a sharded ND
    result" is one of its SJHIP_ERR_ARG cases)."""
    import sjhip
    pad = "x" * 230
    doc = "\n".join('{"pad":"%s","k":%d,"m":{%s}}' % (pad, r % 7, ",".join('"%s%d":%d' % ("abc"[j], r % 5, r + j) for j in range(r % 4)))
                    for r in range(11000)).encode()
    assert len(doc) > 5 << 19
    refused = [lambda c: c.filter_rows(fetch=False), lambda c: c.marshal_rows(fetch=False), lambda c: c.marshal_rows_paths([(b"k",)], fetch=False),
               lambda c: c.marshal_rows_paths([()], names=[b"v"], nulls=True, fetch=False), lambda c: c.serialize(fetch=False),
               lambda c: c.group_path((b"k",), CM.I, fetch=False), lambda c: c.order_path((b"k",), CM.I, fetch=False)]
    many, one = sjhip.Context(0), sjhip.Context(0)
    try:
        with fixtures.nd_shard_limits(2 << 20, 1 << 20):
            many.parse(doc, ndjson=True)
        one.parse(doc, ndjson=True)
        with pytest.raises(sjhip.ParseError):
            many.marshal_rows_paths([(b"k",)], fetch=False)
        assert "shard by shard" in many.last_error()
        info = {}
        for k, (do, name, args) in enumerate(SHARDED_MEMBER_CHAIN):
            if do == "fetch":
                got, want = (CM.device_fetch(c, name, info[name]) for c in (many, one))
                assert CM.differs(got, want) is None, (k, name, CM.differs(got, want))
            elif do == "invalid":
                assert [CM.device_invalid(c, name, args) for c in (many, one)] == [CM.ERR_ARG] * 2, (k, many.last_error(), one.last_error())
            else:
                got, want = (CM.device_call(c, name, args) for c in (many, one))
                assert got[0] == want[0], (k, name, got[0], want[0])
                assert (got[3] is None) == (want[3] is None) and (got[3] is None or CM.differs(got[3], want[3]) is None), (k, name)
                if got[1]:
                    info[got[1]] = got[2]
                if name in CM.SELECTION_CALLS_M and name != "select_records":
                    sizes = (got[0][0], got[0][-1])
                    info["rows"] = sizes
                    assert CM.differs(CM.device_fetch(many, "rows", sizes), CM.device_fetch(one, "rows", sizes)) is None, (k, name)
            for call in refused:
                with pytest.raises(sjhip.ParseError) as e:
                    call(many)
                assert e.value.code == CM.ERR_ARG, (k, many.last_error())
        assert info["parents"] == (11000, 16500) and 5000 < info["column"][0] < 16500  # (the chain ran on rows, and the names were narrowed)
        for what in ("column", "parents"):
            assert CM.differs(CM.device_fetch(many, what, info[what]), CM.device_fetch(one, what, info[what])) is None, what
        assert many.find_path(b"k").tolist() == one.find_path(b"k").tolist()
    finally:
        many.close()
        one.close()
