"""CPU: the generator and the model of tests/chain_model.py alone, over exactly the chains tests/test_gpu_chains.py runs
(chain_model.CHAINS) -- the conditions that keep the GPU test from being vacuous, each printed as measured / required --, and the
model's lifetime table against six short chains whose outcome is written out by hand from the text of csrc/sj_result.h and
include/sjhip.h; the same for chain_model.CHAINS_M, the list of the extended generator (test_7*), and a digest that pins CHAINS."""
import functools

import chain_model as CM
import query_walk as Q
import where_walk as WW
from test_gpu_columns import oracle_walk


@functools.lru_cache(maxsize=None)
def traces():
    return [CM.trace(c[1], c[0], c[2], CM.chain_steps(c)) for c in CM.CHAINS]


def at_least(what, measured, required):
    print("%-86s %5d / %d" % (what, measured, required))
    assert measured >= required, (what, measured, required)


def call_name(step):
    return step[1] if step[0] == "call" else None


def test_the_list_is_spread():
    at_least("chains", len(CM.CHAINS), 32)
    assert CM.STEPS == 16 and all(len(t) == 16 for t in traces())
    for fam in CM.FAMILIES:
        for copy in (True, False):
            at_least("chains of %s, copy=%s" % (fam, copy), sum(c[1] == fam and c[2] == copy for c in CM.CHAINS), 2)
    fresh = sum(c[3] for c in CM.CHAINS)
    assert fresh * 2 == len(CM.CHAINS), fresh
    assert all(c[2] for c, t in zip(CM.CHAINS, traces()) for s, _, _ in t if call_name(s) in ("filter_rows", "serialize"))
    rows = {CM.chain_rows(c[0], c[1]) for c in CM.CHAINS}
    print("row counts:", sorted(rows))
    assert rows >= set(CM.SIZES)
    assert len(CM.DEBUG_CHAINS) == 8 and sum(CM.CHAINS[k][3] for k in CM.DEBUG_CHAINS) >= 2
    twice = [k for k in CM.DEBUG_CHAINS if sum(call_name(s) == "unnest_rows" for s, _, _ in traces()[k]) >= 2]
    at_least("bounds-checked chains that unnest twice", len(twice), 2)
    # Carve::take hands out multiples of 256 bytes: an 8-byte work array that is one element short overlaps its neighbour only where
    # its count is one past a multiple of 32 -- the parents of an unnest_rows right behind a selection of 65, 257 or 1025 rows
    tight = [k for k in CM.DEBUG_CHAINS if any(call_name(s) == "unnest_rows" and j and (traces()[k][j - 1][1] or 0) % 32 == 1 and traces()[k][j - 1][1] > 1
                                               for j, (s, _, _) in enumerate(traces()[k]))]
    at_least("bounds-checked chains that unnest a parent count one past a multiple of 32", len(tight), 2)


def test_1_everything_occurs():
    chains_with = {}
    for k, t in enumerate(traces()):
        for s, _, _ in t:
            key = (s[0], s[1]) if s[0] != "invalid" else ("invalid", s[2][0])
            chains_with.setdefault(key, set()).add(k)
    for name in CM.SELECTION_CALLS + CM.BUILDS:
        at_least("chains with the call %s" % name, len(chains_with.get(("call", name), ())), 4)
    for what in CM.FETCHES:
        at_least("late fetches of %s" % what, len(chains_with.get(("fetch", what), ())), 1)
    at_least("refused fetches", sum(len(v) for k, v in chains_with.items() if k[0] == "refused"), 1)
    for what in CM.TENANTS:
        at_least("refused fetches of the tenant %s" % what, len(chains_with.get(("refused", what), ())), 1)
    for fam in CM.INVALID_FAMILIES:
        at_least("invalid calls of the family %s" % fam, len(chains_with.get(("invalid", fam), ())), 1)
    both = [sum(s[0] == "call" and bool(s[2]) and isinstance(s[2][-1], dict) and s[2][-1].get("fetch") is v for t in traces() for s, _, _ in t)
            for v in (False, True)]
    at_least("builds with fetch=False", both[0], 8)
    at_least("builds with an immediate fetch", both[1], 8)


def fetch_facts():
    """per late fetch: (what, a selection change lay between build and fetch, a larger build of another product lay between: a
    different product or tenant was built between, with more entries (chain_model.size_of) than the fetched thing holds, a further
    different product was built between larger than all ITS earlier builds in the chain -- the build under which an arena that is
    already there has to grow and may move)"""
    out = []
    for t in traces():
        built, grew, largest = {}, [], {}  # what -> (its build's step, its size); the steps at which a product outgrew its earlier builds
        for k, (s, _, sizes) in enumerate(t):
            name = call_name(s)
            for what in ([CM.PUBLISHES[name]] if name in CM.PUBLISHES else []) + (["rows"] if name in CM.SELECTION_CALLS and name != "select_records" else []):
                built[what] = (k, sizes.get(what, 0))
                if what in largest and sizes.get(what, 0) > largest[what]:
                    grew.append((k, what))
                largest[what] = max(largest.get(what, 0), sizes.get(what, 0))
            if s[0] == "fetch":
                what = "marshaled" if s[1] == "marshaled_rows" else s[1]
                at, size = built[what]
                between = [(call_name(b), z) for b, _, z in t[at + 1:k]]
                changed = any(n in CM.SELECTION_CALLS for n, _ in between)
                larger = any(n in CM.PUBLISHES and CM.PUBLISHES[n] != what and z.get(CM.PUBLISHES[n], 0) > size for n, z in between)
                out.append((what, changed, larger, any(at < j < k and other != what for j, other in grew)))
    return out


# The serialized stream holds every word and every string byte of the whole document; nothing a chain builds from the rows of that
# document has more entries, so "a larger build of another product" cannot lie behind it.  What the condition is for -- an arena
# that grows under a live tenant -- is asked of it in the form of the fourth fact instead.
NOTHING_IS_LARGER_THAN = ("serialized",)


def test_2_late_fetches_cross_selection_changes_and_larger_builds():
    facts = fetch_facts()
    for what in CM.PRODUCTS + CM.TENANTS:
        if what != "rows":  # (every selection change is a build of the rows: nothing can lie between)
            at_least("fetches of %s behind a selection change" % what, sum(w == what and c for w, c, _, _ in facts), 3)
        if what not in NOTHING_IS_LARGER_THAN:
            at_least("fetches of %s behind a larger build of another product" % what, sum(w == what and g for w, _, g, _ in facts), 1)
        else:
            at_least("fetches of %s behind a build that outgrew its own arena" % what, sum(w == what and g for w, _, _, g in facts), 1)


def test_3_the_selection_is_seldom_empty_but_sometimes():
    steps = sum(len(t) for t in traces())
    empty = sum(rows == 0 for t in traces() for _, rows, _ in t)
    print("steps on an empty selection: %d of %d (at most a quarter)" % (empty, steps))
    assert empty * 4 <= steps
    at_least("chains in which the selection becomes empty", sum(any(rows == 0 for _, rows, _ in t) for t in traces()), 2)
    builds = sum(t[k - 1][1] == 0 and call_name(t[k][0]) in CM.BUILDS for t in traces() for k in range(1, len(t)))
    at_least("builds on an empty selection", builds, 1)


def test_4_narrowings_in_a_row_and_two_unnests():
    def longest_run(t):
        best = run = 0
        for s, _, _ in t:
            name = call_name(s)
            if name in CM.NARROWINGS:
                run += 1
            elif name in CM.SELECTION_CALLS and name != "unnest_rows":  # a re-selection ends the run (an unnest hands the rows on)
                run = 0
            best = max(best, run)
        return best
    at_least("chains with three narrowings and no re-selection between", sum(longest_run(t) >= 3 for t in traces()), 4)
    at_least("chains in which unnest_rows runs twice", sum(sum(call_name(s) == "unnest_rows" for s, _, _ in t) >= 2 for t in traces()), 2)


def test_5_rebuilt_larger_while_two_others_live():
    hits = 0
    for t in traces():
        first, hit = {}, False
        for s, _, sizes in t:
            what = CM.PUBLISHES.get(call_name(s))
            if what in ("column", "list", "table", "groups", "order", "parents"):
                others = [p for p in sizes if p != what and p != "rows" and p in CM.PRODUCTS]
                if what in first and sizes[what] > first[what] and len(others) >= 2:
                    hit = True
                first.setdefault(what, sizes[what])
        hits += hit
    at_least("chains with a product rebuilt larger while two others live", hits, 4)


# ---- 6. the lifetime table against sj_result.h, by hand --------------------------------------------------------------------------------
# one record, ten rows: r { "items" [ at words 0 .. 4, every row {"id":j,"s":"kJ"} is 10 words, row j's value at word 5 + 10 j
DOC_A = ('{"items":[%s]}' % ",".join('{"id":%d,"s":"k%d"}' % (j, j % 2) for j in range(10))).encode()
# ... and every row {"t":[j]} is 8 words, row j at word 5 + 8 j, its element at 9 + 8 j
DOC_T = ('{"items":[%s]}' % ",".join('{"t":[%d]}' % j for j in range(10))).encode()
OK = 0


def hand_model(doc):
    import oracle_lib as O
    ref = O.parse(doc, ndjson=False, copy_strings=True)
    return CM.Model(Q.Walk(ref.tape, ref.strings, doc), ref)


def test_6a_a_column_is_materialised_data():
    """sj_result.h: "what was built under a selection is materialised data"; select_records is the rows' begin()"""
    m = hand_model(DOC_A)
    assert m.apply(("call", "select_rows", ((b"items",),))).ret == (1, 10)
    assert m.sel == ([0, 10], [5 + 10 * j for j in range(10)], [OK])
    assert m.apply(("call", "extract_path_strings", ((b"s",), {"fetch": False}))).ret == (10, 20)
    assert m.apply(("call", "where_path", ((b"id",), WW.OP_GE_INT, 7, {}))).ret == (1, 3)
    assert m.sel == ([0, 3], [75, 85, 95], [OK])
    m.apply(("call", "select_records", ()))
    assert m.sel is None and not m.exists("rows")
    assert m.apply(("fetch", "column", ())).content == (list(range(0, 22, 2)), b"k0k1" * 5, [OK] * 10)


def test_6b_an_order_survives_and_one_tenant_is_resident():
    """sj_result.h: the order's "row numbers are those of the selection the call left"; "at most one of them is resident"; the text
    of marshal_json has no row offsets (marshaled_by_rows)"""
    m = hand_model(DOC_A)
    m.apply(("call", "select_rows", ((b"items",),)))
    assert m.apply(("call", "marshal_rows", ({"fetch": False},))).ret == (10, 10 * 17 + 9)  # ten texts of 17 bytes, nine newlines
    e = m.apply(("call", "order_path", ((b"id",), CM.I, {"descending": True, "limit": 3, "fetch": False})))
    assert e.ret == (1, 3) and m.sel == ([0, 3], [75, 85, 95], [OK])
    assert m.exists("marshaled") and m.exists("marshaled_rows")
    m.apply(("call", "marshal_json", ({"fetch": False},)))
    assert m.exists("marshaled") and not m.exists("marshaled_rows") and not m.exists("filtered") and not m.exists("serialized")
    assert m.content("marshaled") == DOC_A
    m.apply(("call", "select_records", ()))
    assert m.apply(("fetch", "order", ())).content == ([2, 1, 0], [9, 8, 7], [OK, OK, OK])


def test_6c_an_argument_error_touches_nothing_and_the_parents_outlive_the_rows():
    """sjhip.h: "SJHIP_ERR_ARG ... nothing touched (the selection and the previous parents stay as they were)"; sj_result.h: the
    parents are "materialised like the other two\""""
    m = hand_model(DOC_T)
    m.apply(("call", "select_rows", ((b"items",),)))
    assert m.apply(("call", "unnest_rows", ((b"t",),))).ret == (1, 10, 10)
    assert m.sel == ([0, 10], [9 + 8 * j for j in range(10)], [OK])
    assert m.apply(("invalid", "unnest_rows", ("path17", (b"t",), (b"t",)))).error == CM.ERR_ARG
    assert m.sel == ([0, 10], [9 + 8 * j for j in range(10)], [OK]) and m.exists("parents")
    m.apply(("call", "select_records", ()))
    assert m.apply(("refused", "rows", ())).error == CM.ERR_ARG
    assert m.apply(("fetch", "parents", ())).content == (list(range(11)), list(range(10)), [OK] * 10)


# one record, one map of ten members: r { "m" { at words 0 .. 4; member j is "<name>" (two words) and {"id":j,"t":[j]} (12 words):
# its value at word 7 + 14 j, the one element of its "t" at 15 + 14 j
NAMES_M = [b"a0", b"b1", b"a2", b"b3", b"a4", b"b5", b"a6", b"b7", b"a8", b"b9"]
DOC_M = ('{"m":{%s}}' % ",".join('"%s":{"id":%d,"t":[%d]}' % (n.decode(), j, j) for j, n in enumerate(NAMES_M))).encode()


def test_6d_the_names_follow_the_rows_through_two_narrowings():
    """sjhip.h: the name calls take "the one sjhip_unnest_members left, or what sjhip_where_*, sjhip_where_row_names and the limit
    of sjhip_order_* narrowed it to"; "the name of a row is read from the two tape words in front of its value"; an order keeps
    "the selection in document order\""""
    m = hand_model(DOC_M)
    assert m.apply(("call", "unnest_members", ((b"m",),))).ret == (1, 1, 10)
    assert m.sel == ([0, 10], [7 + 14 * j for j in range(10)], [OK]) and m.members
    assert m.apply(("call", "where_row_names", (WW.OP_PREFIX_STRING, b"a", {}))).ret == (1, 5)
    assert m.sel == ([0, 5], [7 + 14 * j for j in (0, 2, 4, 6, 8)], [OK]) and m.members
    e = m.apply(("call", "order_path", ((b"id",), CM.I, {"descending": True, "limit": 3, "fetch": False})))
    assert e.ret == (1, 3) and m.sel == ([0, 3], [63, 91, 119], [OK]) and m.members
    e = m.apply(("call", "extract_row_names", ({},)))
    assert e.ret == (3, 6) and e.content == ([0, 2, 4, 6], b"a4a6a8", [OK] * 3)


def test_6e_the_names_outlive_the_member_rows_and_the_name_call_is_refused():
    """sjhip.h: "After sjhip_select_rows, sjhip_unnest_rows, sjhip_select_records or a parse they return SJHIP_ERR_ARG, touch
    nothing"; the names are "the product of sjhip_extract_path_strings": materialised data"""
    m = hand_model(DOC_M)
    m.apply(("call", "unnest_members", ((b"m",),)))
    assert m.apply(("call", "extract_row_names", ({"fetch": False},))).ret == (10, 20)
    assert m.apply(("call", "unnest_rows", ((b"t",),))).ret == (1, 10, 10)
    assert m.sel == ([0, 10], [15 + 14 * j for j in range(10)], [OK]) and not m.members
    assert m.apply(("invalid", "extract_row_names", ("not_members", Q.OP_EQ_STRING, b"a0"))).error == CM.ERR_ARG
    assert m.sel == ([0, 10], [15 + 14 * j for j in range(10)], [OK]) and not m.members
    assert m.apply(("fetch", "column", ())).content == (list(range(0, 22, 2)), b"".join(NAMES_M), [OK] * 10)
    try:
        m.apply(("call", "extract_row_names", ({},)))  # (the model itself refuses to be asked)
        assert False
    except AssertionError:
        pass


def test_6f_a_projection_leaves_the_table_and_yields_to_marshal_json():
    """sjhip.h, sjhip_marshal_rows_paths: "The selection, the string column, the list column and the table stay as they are";
    the result is "the marshaled product of the context with the row offsets behind it"; sjhip_fetch_marshaled_rows is
    "SJHIP_ERR_ARG after sjhip_marshal_json, whose text has no rows\""""
    m = hand_model(DOC_A)
    m.apply(("call", "select_rows", ((b"items",),)))
    assert m.apply(("call", "extract_table", ([((b"id",), CM.I), ((b"s",), CM.S)], {"fetch": False}))).ret == (10, [0, 20])
    e = m.apply(("call", "marshal_rows_paths", ([(b"s",), (b"nope",), (b"id",)], [b"", b"n", b'q"'], True, {})))
    rows = [b'{"":"k%d","n":null,"q\\"":%d}' % (j % 2, j) for j in range(10)]
    assert e.ret == (10, len(b"\n".join(rows))) and e.content[1] == b"\n".join(rows) and e.content[2] == list(range(0, 271, 27))
    assert m.exists("marshaled_rows") and m.content("marshaled_rows") == (b"\n".join(rows), list(range(0, 271, 27)))
    m.apply(("call", "marshal_json", ({"fetch": False},)))
    assert m.apply(("refused", "marshaled_rows", ())).error == CM.ERR_ARG
    assert m.apply(("fetch", "marshaled", ())).content == DOC_A
    assert m.apply(("fetch", "table", ())).content == [(list(range(10)), [OK] * 10), (list(range(0, 22, 2)), b"k0k1" * 5, [OK] * 10)]
    assert m.sel == ([0, 10], [5 + 10 * j for j in range(10)], [OK])


def test_the_script_replays_and_the_comparison_has_teeth():
    steps = CM.chain_steps(CM.CHAINS[0])
    text = CM.script(steps, "h")
    assert text.count("\n") == len(steps) + 2 and "CM.device_call(ctx, " in text
    assert CM.differs(([0, 1], b"ab", [0]), ([0, 1], b"ab", [0])) is None
    assert "entry 1" in CM.differs(([0, 1], b"ab", [0]), ([0, 2], b"ab", [0]))
    assert CM.differs(("agg", CM.I, 1, [1], 0, 0, 2 ** 70, None), ("agg", CM.I, 1, [1], 0, 0, 2 ** 70 + 1, None)) is not None
    assert CM.differs(("agg", CM.F, 1, [1], 0, 0, 0.1 + 0.2, None), ("agg", CM.F, 1, [1], 0, 0, 0.3, None)) is not None
    assert CM.differs(("agg", CM.F, 1, [1], 0, 0, 0.1 + 0.2, None), ("agg", CM.F, 1, [1], 0, 0, 0.3, 1e-15)) is None


def test_the_canonical_forms_have_teeth():
    """the forms of device_fetch and differs: a grouping's float sums are compared -- by the bound, or as bits -- and everything
    around them exactly; _bits keeps every bit of the 1-byte and 8-byte columns and refuses other widths"""
    import numpy as np
    sums = [[2, 1], [0, 0], [CM.CW.f2bits(0.75), CM.CW.f2bits(0.3)], [0, 0], [0, 0], [9, 9]]

    def one(total0, codes=(0, 1, 0), count=2, bound=None):
        aggs = [list(a) for a in sums]
        aggs[0][0], aggs[2][0] = count, CM.CW.f2bits(total0)
        return ("one", [b"a", b"b"], [0, 1], [2, 1], list(codes), [0, 0, 0], aggs, [(0.75, bound), (0.3, None)])
    want = one(0.75)
    got = one(0.75)[:7] + (None,)  # (the device's form carries no sums of the model)
    assert CM.differs(got, want) is None
    assert "group 0" in CM.differs(one(0.7500000000000001)[:7] + (None,), want)
    assert CM.differs(one(0.7500000000000001)[:7] + (None,), one(0.75, bound=1e-12)) is None
    assert "group 0" in CM.differs(one(0.76)[:7] + (None,), one(0.75, bound=1e-12))
    assert CM.differs(one(0.75, codes=(0, 1, 1))[:7] + (None,), want) is not None   # beside the sums: exactly
    assert CM.differs(one(0.75, count=3)[:7] + (None,), want) is not None           # ... the other aggregate arrays as well
    many = ("many", [[b"a"], [5]], [[1], [1]], [[0], [0]], [0], [1], [0], [[[1], [0], [7], [0], [7], [7]]])
    assert CM.differs(many, many) is None
    worse = ("many", [[b"a"], [5]], [[1], [1]], [[0], [0]], [0], [1], [0], [[[1], [0], [8], [0], [7], [7]]])
    assert CM.differs(worse, many) is not None
    assert CM._bits(np.array([-1, 2], dtype=np.int64)) == [CM.U64, 2] and CM._bits(np.array([-0.0])) == [1 << 63]
    assert CM._bits(np.array([1, 255], dtype=np.uint8)) == [1, 255]
    for dt in (np.uint32, np.int16, np.float32):
        try:
            CM._bits(np.zeros(2, dtype=dt))
            assert False, dt
        except ValueError:
            pass


# ---- the existing chains are pinned ------------------------------------------------------------------------------------------------------
# sha256 over chain_model.script(chain_steps(c)) of all of CHAINS, in order, computed before the generator learned the extended
# draws: the 64 seeded chains are exactly the ones that were there
CHAINS_DIGEST = "06cc5890f6c2ea8a507fc3e2ff263b04943e4d5c9fca70efba4e225682b20c70"


def test_the_first_chains_are_the_ones_they_were():
    import hashlib
    h = hashlib.sha256()
    for c in CM.CHAINS:
        h.update(CM.script(CM.chain_steps(c)).encode())
    assert h.hexdigest() == CHAINS_DIGEST


# ---- 7. the extended list: member rows, row names, projected rows, the two readers ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def traces_m():
    return [CM.trace_m(c) for c in CM.CHAINS_M]


def walked():
    """per chain, per step: the trace's dict and, kept along the chain, since: the selection calls since the last call that
    replaced or dropped the selection (that call first; [] before any), this step included; before: the same in front of the step; cleared: the call that last cleared a member selection
    (None while members are in force or never were)"""
    out = []
    for t in traces_m():
        since, cleared, steps = [], None, []
        for f in t:
            name, before = call_name(f["step"]), since
            if name in CM.SELECTION_CALLS_M:
                if name in CM.NARROWINGS_M:
                    since = since + [f["step"]]
                else:
                    since = [f["step"]]
                if name == "unnest_members":
                    cleared = None
                elif name in CM.CLEARS_MEMBERS and f["was_members"]:
                    cleared = name
            steps.append(dict(f, since=since, before=before, cleared=cleared))
        out.append(steps)
    return out


def limited(step):
    return step[1].startswith("order_") and step[2][-1].get("limit", 0) > 0


def test_7_the_extended_list_is_spread():
    at_least("extended chains", len(CM.CHAINS_M), 48)
    assert len(CM.CHAINS_M) <= 96 and len(set(CM.CHAINS_M)) == len(CM.CHAINS_M)
    assert all(len(t) == CM.STEPS for t in traces_m())
    for fam in CM.FAMILIES_M:
        for copy in (True, False):
            at_least("extended chains of %s, copy=%s" % (fam, copy), sum(c[1] == fam and c[2] == copy for c in CM.CHAINS_M), 2)
    assert sum(c[3] for c in CM.CHAINS_M) * 2 == len(CM.CHAINS_M)
    assert all(c[2] for c, t in zip(CM.CHAINS_M, traces_m()) for f in t if call_name(f["step"]) in ("filter_rows", "serialize"))
    rows = {CM.chain_rows(c[0], c[1]) for c in CM.CHAINS_M}
    print("row counts:", sorted(rows))
    assert rows >= set(CM.SIZES)
    assert len(CM.DEBUG_CHAINS_M) == len(set(CM.DEBUG_CHAINS_M)) == 8
    at_least("bounds-checked extended chains on a fresh context", sum(CM.CHAINS_M[k][3] for k in CM.DEBUG_CHAINS_M), 2)
    twice = [k for k in CM.DEBUG_CHAINS_M if sum(call_name(f["step"]) == "unnest_members" for f in traces_m()[k]) >= 2]
    at_least("bounds-checked extended chains that draw unnest_members twice", len(twice), 2)
    # (the reason test_the_list_is_spread gives for unnest_rows: the parents' work arrays are carved in multiples of 256 bytes)
    tight = [k for k in CM.DEBUG_CHAINS_M if any(call_name(f["step"]) == "unnest_members" and (f["rows_before"] or 0) % 32 == 1 and f["rows_before"] > 1
                                                 for f in traces_m()[k])]
    at_least("bounds-checked extended chains with a parent count one past a multiple of 32 in front of unnest_members", len(tight), 2)


def test_7a_every_call_occurs():
    chains_with = {}
    for k, t in enumerate(traces_m()):
        for f in t:
            chains_with.setdefault(f["step"][:2], set()).add(k)
    for name in CM.NEW_CALLS + CM.SELECTION_CALLS + CM.BUILDS:
        at_least("extended chains with the call %s" % name, len(chains_with.get(("call", name), ())), 4)


def test_7b_names_behind_narrowed_member_rows():
    hits = {"where_path or where_paths": 0, "where_row_names": 0, "order_path with a limit": 0, "order_path_strings with a limit": 0,
            "order_paths with a limit": 0, "two or more narrowings in a row": 0}
    for steps in walked():
        for f in steps:
            if call_name(f["step"]) in ("extract_row_names", "where_row_names") and f["was_members"]:
                behind = [s for s in f["since"] if s is not f["step"]]
                if not behind or behind[0][1] != "unnest_members":
                    continue
                names = [s[1] for s in behind[1:]]
                hits["where_path or where_paths"] += bool({"where_path", "where_paths"} & set(names))
                hits["where_row_names"] += "where_row_names" in names
                for o in ("order_path", "order_path_strings", "order_paths"):
                    hits[o + " with a limit"] += any(s[1] == o and limited(s) for s in behind[1:])
                hits["two or more narrowings in a row"] += len(names) >= 2
    for what, need in (("where_path or where_paths", 3), ("where_row_names", 3), ("order_path with a limit", 1), ("order_path_strings with a limit", 1),
                       ("order_paths with a limit", 1), ("two or more narrowings in a row", 3)):
        at_least("name calls on member rows narrowed by %s" % what, hits[what], need)


def test_7c_invalid_calls_in_every_position():
    places = {"no selection at all": 0, "select_rows after members": 0, "unnest_rows after members": 0, "select_records after members": 0,
              "a narrowing of an array selection": 0}
    others = {"name_op": 0}
    others.update({"project " + form: 0 for form in CM.PROJECT_FORMS})
    for steps in walked():
        for f in steps:
            do, name, args = f["step"]
            if do != "invalid":
                continue
            if args[0] == "not_members":
                assert not f["members"]
                places["no selection at all"] += f["rows"] is None
                if f["cleared"]:
                    places[f["cleared"] + " after members"] += 1
                elif f["rows"] is not None and f["since"] and f["since"][-1][1] in CM.NARROWINGS:
                    places["a narrowing of an array selection"] += 1
            elif args[0] == "name_op":
                others["name_op"] += 1
            elif args[0] == "project":
                others["project " + args[1]] += 1
    for what, n in list(places.items()):
        at_least("not_members invalid calls behind %s" % what, n, 1)
    for what, n in others.items():
        at_least("invalid calls of the family %s" % what, n, 1)


def late_fetches_m():
    """per late fetch of the extended chains: (what, the call that published it, the steps between that call and the fetch)"""
    out = []
    for t in traces_m():
        built = {}
        for k, f in enumerate(t):
            do, name, _ = f["step"]
            if do == "call" and name in CM.PUBLISHES:
                built[CM.PUBLISHES[name]] = k
            if do == "call" and name in CM.SELECTION_CALLS_M and name != "select_records":
                built["rows"] = k
            if do == "fetch":
                what = "marshaled" if name == "marshaled_rows" else name
                out.append((name, call_name(t[built[what]]["step"]), t[built[what]], t[built[what] + 1:k]))
    return out


def test_7d_late_fetches_of_names_parents_and_beside_a_projection():
    late = late_fetches_m()
    cleared = sum(what == "column" and by == "extract_row_names" and any(call_name(f["step"]) in CM.CLEARS_MEMBERS and f["was_members"] for f in between)
                  for what, by, _, between in late)
    at_least("late fetches of names behind a selection change that cleared members", cleared, 3)
    replaced = 0
    for t in traces_m():
        for k, f in enumerate(t):
            if f["step"][:2] == ("fetch", "column") and f["origin"]["column"] == "extract_path_strings":
                calls = [call_name(g["step"]) for g in t[:k] if call_name(g["step"]) in ("extract_row_names", "extract_path_strings")]
                replaced += len(calls) >= 2 and calls[-2] == "extract_row_names"
    at_least("late fetches of column behind an extract_path_strings that replaced names", replaced, 1)
    at_least("late fetches of parents published by unnest_members", sum(what == "parents" and by == "unnest_members" for what, by, _, _ in late), 3)
    larger = 0
    for product in ("table", "column", "list"):
        hits = [(at, [f for f in between if call_name(f["step"]) == "marshal_rows_paths"]) for what, _, at, between in late if what == product]
        hits = [(at, ps) for at, ps in hits if ps]
        at_least("late fetches of %s with marshal_rows_paths between build and fetch" % product, len(hits), 3)
        if product == "table":
            larger = sum(any((p["rows"] or 0) * len(p["step"][2][0]) > (at["rows"] if at["rows"] is not None else 0) * len(at["step"][2][0]) for p in ps)
                         for at, ps in hits if at["rows"] is not None)
    at_least("... of table where the projection has more cells (rows x columns) than the table", larger, 1)
    projected = [(between) for what, by, _, between in late if what == "marshaled_rows" and by == "marshal_rows_paths"]
    at_least("late fetches of marshaled_rows that deliver a projection", len(projected), 3)
    at_least("... behind a selection change", sum(any(call_name(f["step"]) in CM.SELECTION_CALLS_M for f in between) for between in projected), 1)
    refused_tenant = refused_rows = 0
    for t in traces_m():
        for k, f in enumerate(t):
            do, name, _ = f["step"]
            if do == "refused" and name in ("filtered", "serialized") and f["origin"].get("marshaled") == "marshal_rows_paths":
                refused_tenant += 1
            if do == "refused" and name == "marshaled_rows" and f["origin"].get("marshaled") == "marshal_json":
                refused_rows += any(call_name(g["step"]) == "marshal_rows_paths" for g in t[:k])
    at_least("refused fetches of filtered or serialized behind a projection", refused_tenant, 1)
    at_least("refused fetches of marshaled_rows behind marshal_json after a projection", refused_rows, 1)


def test_7e_member_rows_twice_mixed_and_feeding_every_consumer():
    w = walked()
    at_least("extended chains in which unnest_members runs twice", sum(sum(call_name(f["step"]) == "unnest_members" for f in t) >= 2 for t in w), 2)
    at_least("unnest_rows directly behind member rows", sum(call_name(f["step"]) == "unnest_rows" and f["was_members"] for t in w for f in t), 2)
    at_least("unnest_members behind unnest_rows", sum(call_name(f["step"]) == "unnest_members" and bool(f["before"]) and f["before"][0][1] == "unnest_rows"
                                                      for t in w for f in t), 2)
    for name in CM.BUILDS + ("marshal_rows_paths", "aggregate_path_records"):
        at_least("calls of %s on a member selection" % name, sum(call_name(f["step"]) == name and f["was_members"] for t in w for f in t), 1)
    empty = [(k, j) for k, t in enumerate(w) for j, f in enumerate(t)
             if call_name(f["step"]) == "unnest_members" and f["rows"] == 0 and f["ok_parents"] == 0]
    at_least("member selections that are empty because no parent was OK", len(empty), 2)
    at_least("builds on such a selection", sum(call_name(w[k][j + 1]["step"]) in CM.BUILDS_M for k, j in empty if j + 1 < len(w[k])), 1)
    steps = sum(len(t) for t in w)
    on_empty = sum(f["rows"] == 0 for t in w for f in t)
    print("steps on an empty selection: %d of %d (at most a quarter)" % (on_empty, steps))
    assert on_empty * 4 <= steps


def test_7f_the_catalog_names():
    for what in ("duplicate", "empty", "escaped", "long"):
        n = sum(c[1] == "catalog" and any(what in f["names"] for f in t) for c, t in zip(CM.CHAINS_M, traces_m()))
        at_least("catalog chains whose member rows include a name that is %s" % what, n, 2)
