"""CPU: the generator and the model of tests/chain_model.py alone, over exactly the chains tests/test_gpu_chains.py runs
(chain_model.CHAINS) -- the conditions that keep the GPU test from being vacuous, each printed as measured / required --, and the
model's lifetime table against three short chains whose outcome is written out by hand from the text of csrc/sj_result.h."""
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
