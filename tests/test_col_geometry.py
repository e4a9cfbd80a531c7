"""CPU: tests/col_geometry.py agrees with the source text of csrc/query.hip and csrc/sj_tapewalk.h, every case of
tests/test_gpu_column_seams.py lies on the cut it is named for (shown from the oracle's tape through the model's trace), the
builders' expectations are what column_walk / list_walk make of the oracle's parse, the unmutated host model delivers them, and
every mutation of the model is told from it by a named case."""
import os
import re

import pytest

import col_geometry as G
import column_walk as CW
import list_walk as LW

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simdjson-go_amd", "csrc")
ALL = G.all_cases()
BY_FAMILY = {f: [c for c in ALL if c.family == f] for f in G.MODES}


@pytest.fixture(scope="module")
def walks():
    cache = {}

    def get(case, copy=True):
        key = (case.name, copy)
        if key not in cache:
            cache[key] = G.walk(case.doc, copy, case.select)
        return cache[key]
    return get


# ---- the constants and the launch shapes are the sources' ---------------------------------------------------------------------------
def test_mirror_constants_are_the_sources():
    src = open(os.path.join(CSRC, "query.hip")).read()
    tw = open(os.path.join(CSRC, "sj_tapewalk.h")).read()

    def one(pattern, text=src, count=None):
        m = re.findall(pattern, text)
        assert len(m) >= 1 and len(set(m)) == 1 and (count is None or len(m) == count), (pattern, m)
        return m[0]

    assert int(one(r"static constexpr u64 COL_SHORT = (\d+);")) == G.COL_SHORT
    assert int(one(r"static constexpr u64 LIST_SHORT = (\d+);")) == G.LIST_SHORT
    assert int(one(r"TW_THREADS = (\d+),", tw)) == G.QT
    assert int(one(r"static constexpr int QT = TW_THREADS, QI = (\d+), QTILE = QT \* QI;", tw)) == G.QI and G.QTILE == G.QT * G.QI
    # the routes: one test per kernel, each against its constant
    one(r"wide = len > COL_SHORT;", count=2)                      # k_q_col_gather (and the group keys, which share the copy)
    one(r"wide = close - v - 1 > 2 \* LIST_SHORT;", count=1)      # k_q_list_measure: words
    one(r"wide = cnt > LIST_SHORT;", count=1)                     # k_q_list_gather_num: elements
    one(r"wide = !CVT && cnt > LIST_SHORT;", count=1)             # list_gather_strings: elements, AsString alone
    one(r"if \(len > COL_SHORT\) \{", count=1)                    # the waiting lane
    one(r"if \(len && len <= COL_SHORT\) copy_bytes", count=1)    # AsString's long arrays: the lane's side ...
    one(r"wave_copy_strings\(q, data, len > COL_SHORT, mine, len, w, lane\);", count=1)  # ... and the wave's
    # the wave steps: 64 bytes, 64 elements (128 words), 64 lengths
    assert int(one(r"str_bytes\(q, wave_bcast\(w, j\), lj\), lj, \(u64\)lane, (\d+)\);")) == G.WAVE
    assert int(one(r"for \(u64 g = v \+ 1; g < close; g \+= (\d+)\)")) == 2 * G.WAVE
    assert int(one(r"for \(u64 k = \(u64\)lane; k < nj; k \+= (\d+)\)")) == G.WAVE
    assert int(one(r"for \(u64 g = 0; g < nj; g \+= (\d+)\)")) == G.WAVE
    assert one(r"if \(bad\) return __shfl\(st, (__ffsll\(\(unsigned long long\)bad\) - 1), 64\);")  # the lowest lane of the ballot
    assert one(r"base \+= wave_bcast\(incl, (63)\);") == "63"
    # one thread per record in blocks of 256; the measures have thread n, the gathers do not; the scan has n + 1 entries
    kernels = ("k_q_col_len", "k_q_col_gather", "k_q_list_measure", "k_q_list_measure_cvt", "k_q_list_gather_num", "k_q_list_gather_str",
               "k_q_list_gather_cvt")
    for k in kernels:
        assert int(one(r"__launch_bounds__\((\d+)\) void %s\(" % k)) == G.BLOCK, k
    assert one(r"hipLaunchKernelGGL\(k_q_col_len, dim3\(\((n \+ 1u \+ 255\) / 256)\), dim3\(256\)") and G.measure_blocks(256) == 2
    assert one(r"hipLaunchKernelGGL\(k_q_col_gather, dim3\(\((n \+ 255\) / 256)\), dim3\(256\)") and G.gather_blocks(256) == 1
    assert one(r"const dim3 grid\(\(n \+ 1u \+ 255\) / 256\), block\(256\);\n.*\n\s+if \(mode == LIST_CVT\) hipLaunchKernelGGL\((k_q_list_measure_cvt), grid, block")
    assert one(r"const dim3 grid\(\(n \+ 255\) / 256\), block\(256\);\n\s+if \(!strings\(\)\)\n\s+hipLaunchKernelGGL\((k_q_list_gather_num), grid, block")
    assert one(r"static u32 tiles_of\(u32 n\) \{ return (\(n \+ 1u \+ QTILE - 1\) / QTILE); \}")
    assert one(r"if \(r == q_rows\(q\)\) c\.off\[r\] = (0);") == "0" and one(r"\} else if \(r == q_rows\(q\)\) \{\n\s+c\.cnt\[r\] = (0);") == "0"
    assert [G.scan_tiles(n) for n in (1022, 1023, 1024, 2047, 2048)] == [1, 1, 2, 2, 3]
    assert [G.measure_blocks(n) - G.gather_blocks(n) for n in (255, 256, 257, 1024, 2047, 2048)] == [0, 1, 0, 1, 0, 1]
    assert G.string_route(32) == (G.LANE, 0) and [G.string_route(n) for n in (33, 64, 65, 128, 129)] == [(G.WIDE, k) for k in (1, 1, 2, 2, 3)]
    assert [G.list_measure_route(w) for w in (32, 33, 34)] == [G.LANE, G.WIDE, G.WIDE]
    assert [G.list_gather_route(e) for e in (16, 17)] == [G.LANE, G.WIDE] and [G.steps(e) for e in (64, 65, 128, 129)] == [1, 2, 2, 3]


# ---- the case lists -------------------------------------------------------------------------------------------------------------------
def test_case_lists_hold_what_they_are_named_for_and_stay_small(walks):
    assert len({c.name for c in ALL}) == len(ALL)
    for c in ALL:
        assert len(c.doc) < 300000 and len(c.rows) < 2100, c.name
        assert len(walks(c).records()) == len(c.rows), c.name
    names = " | ".join(c.name for c in ALL)
    for n in G.STR_LENS:
        assert "strings: %d bytes at lanes" % n in names
    for n in G.LIST_LENS:
        assert "numbers: %d elements at lanes" % n in names
    for n in G.COUNTS:
        assert "strings: %d rows" % n in names and "numbers: %d rows" % n in names
    for n in G.LSTR_LENS:
        assert "strings of %d bytes" % n in names
    assert G.STR_LENS == (0, 1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 225)
    assert G.LIST_LENS == (0, 1, 15, 16, 17, 63, 64, 65, 80, 127, 128, 129, 192, 193)
    assert G.COUNTS == (1, 63, 64, 65, 255, 256, 257, 1022, 1023, 1024, 1025, 2047, 2048)
    assert len(G.FAIL_AT) == 41 and {f for _, f in G.FAIL_AT} >= {0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 199}
    for e, f in G.FAIL_AT:
        assert f < e and e in (16, 17, 64, 65, 129, 200)
    # the lookalikes are tags, the longest texts are the longest, the boxes have the words they say
    assert all(chr(v >> 56) == t for t, v in G.RAW.items())
    assert (len(G.I64MIN.text), len(G.U64MAX.text), len(G.FLTMAX.text)) == (20, 20, 24)
    w = G.walk(b'{"a":[[],[1],{"a":[1,2,3]},{},%s]}' % G.OBJ40.text.encode())
    v, i, got = w.find_path(0, [b"a"]), 0, []
    i = v + 1
    while chr(w.t[i] >> 56) != "]":
        got.append(w.skip(i) - i)
        i = w.skip(i)
    assert got == [e.words for e in (G.EMPTY_ARR, G.ONE_ARR, G.OBJ12, G.EMPTY_OBJ, G.OBJ40)] == [2, 4, 12, 2, 40]


def check_claims(case, mode, trace):
    for r, claim in case.claim.items():
        if isinstance(r, str):  # a claim about the whole trace
            key, _, only = r.partition("@")
            if only in ("", mode):
                assert trace[key] == claim, (case.name, mode, key, trace[key], claim)
            continue
        assert G.place(r) == {k: claim[k] for k in ("lane", "wave", "block", "tile")}, (case.name, r)
        for k, want in claim.items():
            key, _, only = k.partition("@")
            if key in ("lane", "wave", "block", "tile") or only not in ("", mode):
                continue
            assert trace[key][r] == want, (case.name, mode, r, key, trace[key][r], want)


@pytest.mark.parametrize("family", sorted(G.MODES))
def test_every_case_on_its_branch_and_the_model_delivers_the_expectation(walks, family):
    """from the oracle's tape: the trace of the unmutated model shows the route, step, lane and rounds the case claims, and its
    arrays are the builder's expectation"""
    for c in BY_FAMILY[family]:
        for copy in (True, False) if family != "numbers" else (True,):
            for mode in G.MODES[family]:
                got = G.model(walks(c, copy), c.path, mode)
                assert G.differs(got, G.expect(c, mode)) is None, (c.name, mode, copy, G.differs(got, G.expect(c, mode)))
                check_claims(c, mode, got["trace"])


def test_the_claims_cover_the_cuts():
    """the routes, lanes and steps the lists are meant to reach are claimed by some case (the claims themselves are checked above)"""
    routes = {c["route"] for case in BY_FAMILY["strings"] for c in case.claim.values()}
    assert routes >= {(G.LANE, 0), (G.WIDE, 1), (G.WIDE, 2), (G.WIDE, 3), (G.WIDE, 4)}
    where = {(c["route"][0], c["lane"], c["wave"]) for case in BY_FAMILY["strings"] for c in case.claim.values()}
    assert where >= {(rt, lane, wv) for rt in (G.LANE, G.WIDE) for lane in (0, 1, 62, 63) for wv in (0, 3)}
    tiles = {(c["tile"], r % G.QTILE) for case in BY_FAMILY["strings"] for r, c in case.claim.items() if c["route"][0] == G.WIDE}
    assert tiles >= {(0, G.QTILE - 1), (1, 0)}
    num = [c for case in BY_FAMILY["numbers"] for r, c in case.claim.items()]
    assert {(c["measure"], c["gather@int"]) for c in num} == {(G.LANE, G.LANE), (G.WIDE, G.WIDE), (G.WIDE, G.LANE)}
    fails = {c["fail@uint"] for c in num if c["measure"] == G.WIDE and c["fail@uint"] is not None}
    assert fails >= {(0, 0), (0, 1), (0, 15), (0, 16), (0, 17), (0, 63), (1, 0), (1, 1), (1, 63), (2, 0), (3, 7)}
    assert {c["fail@uint"] for c in num if c["measure"] == G.LANE} >= {None, 0, 1, 15}
    rounds = [tuple(rd) for case in BY_FAMILY["list_strings"] for k in ("rounds@list_str", "rounds@list_cvt") for rd in case.claim[k].values()]
    assert ((5, 9),) in rounds and ((7, 8, 20), (7,)) in rounds and ((31,),) * 16 in rounds and any(r[:1] == ((0, 63),) for r in rounds)
    longs = {x for case in BY_FAMILY["list_strings"] for c in case.claim.values() if isinstance(c, dict) and "long@list_str" in c
             for x in c["long@list_str"]}
    assert longs >= {(0, 0), (0, 63), (1, 0), (1, 63), (2, 0)}
    for fam in G.MODES:  # the partial wave, entry n in a block of its own, the scan tiles
        ns = {len(c.rows) for c in BY_FAMILY[fam]}
        assert ns >= {65, 127}
        if fam != "list_strings":
            assert ns >= set(G.COUNTS)


# ---- the expectation is the walkers' ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(G.MODES))
def test_expectation_equals_the_walkers(walks, family):
    for c in BY_FAMILY[family]:
        w = walks(c)
        for mode in G.MODES[family]:
            e = G.expect(c, mode)
            if family == "strings":
                assert (e["off"], e["data"], e["status"]) == CW.string_column(w, c.path, mode == "strings_cvt"), (c.name, mode)
            elif family == "numbers":
                assert (e["off"], e["vals"], e["status"]) == LW.list_column(w, c.path, G.KIND[mode]), (c.name, mode)
            else:
                assert (e["off"], e["soff"], e["data"], e["status"]) == LW.list_string_column(w, c.path, mode == "list_cvt"), (c.name, mode)


# ---- every mutation is caught ---------------------------------------------------------------------------------------------------------
# mutation -> (the case that tells it from the kernels, the mode, what differs: a fetched array, or the route alone -- a kernel
# that takes the other route of a cut correctly fetches the same arrays, so only the trace can show it)
CAUGHT = {
    "COL_SHORT - 1 in the lane's test": ("strings: 32 bytes at lanes 0, 1, 62, 63 of waves 0 and 3", "strings", "data"),
    "COL_SHORT + 1 in the wave's test": ("strings: 33 bytes at lanes 0, 1, 62, 63 of waves 0 and 3", "strings", "data"),
    "LIST_SHORT - 1 in the lane's test": ("numbers: 16 elements at lanes 0 and 63", "int", "off"),
    "LIST_SHORT + 1 in the wave's test": ("numbers: 17 elements at lanes 0 and 63", "int", "off"),
    "a wave step of 63": ("list strings: every element count with strings of 1 bytes", "list_str", "soff"),
    "entry n not written": ("strings: 256 rows", "strings", "totals"),
    "the highest failing lane": ("numbers: two failures of different status, in one step and in two, both orders", "uint", "status"),
    "shifted words trusted behind a one-word element": ("numbers: true at every (E, f), payloads that look like l behind it", "int", "off"),
    "the measure routed by elements": ("numbers: words say wave, elements say lane", "int", "route"),
    "base not carried between AsString steps": ("list strings: every element count with strings of 1 bytes", "list_str", "soff"),
    "the lanes without a record left out of the step loop": ("strings: 65 rows, the last one wide in a partial wave", "strings", "data"),
}
ALSO = [  # the same mutations in the other products that share the cut
    ("COL_SHORT - 1 in the lane's test", "list strings: every element count with strings of 32 bytes", "list_str", "data"),
    ("COL_SHORT + 1 in the wave's test", "list strings: every element count with strings of 33 bytes", "list_cvt", "data"),
    ("LIST_SHORT - 1 in the lane's test", "list strings: every element count with strings of 1 bytes", "list_str", "off"),
    ("LIST_SHORT + 1 in the wave's test", "list strings: every element count with strings of 1 bytes", "list_str", "off"),
    ("entry n not written", "numbers: 1024 rows", "float", "totals"),
    ("entry n not written", "numbers: 2048 rows", "uint", "totals"),
    ("the lanes without a record left out of the step loop", "numbers: 65 rows, the last array wide in a partial wave", "int", "vals"),
    ("the lanes without a record left out of the step loop", "list strings: 127 rows, a waiting lane and a wide array in a partial wave", "list_str", "soff"),
    ("the lanes without a record left out of the step loop", "list strings: 127 rows, a waiting lane and a wide array in a partial wave", "list_cvt", "data"),
]


def mutated(walks, mutation, name, mode):
    c = G.CASES[name]
    return c, G.model(walks(c), c.path, mode, **G.MUTATIONS[mutation])


def test_every_mutation_is_caught_by_a_named_case(walks):
    assert set(CAUGHT) == set(G.MUTATIONS)
    for mutation, (name, mode, what) in CAUGHT.items():
        c, got = mutated(walks, mutation, name, mode)
        first = G.differs(got, G.expect(c, mode))
        if what == "route":  # the arrays are the same: the case pins the route through its claim
            assert first is None
            with pytest.raises(AssertionError):
                check_claims(c, mode, got["trace"])
        else:
            assert what in G.differing(got, G.expect(c, mode)), (mutation, name, first)
        print("%-55s caught by %r (%s: %s)" % (mutation, name, mode, what))
    for mutation, name, mode, what in ALSO:
        c, got = mutated(walks, mutation, name, mode)
        assert what in G.differing(got, G.expect(c, mode)), (mutation, name, mode, G.differing(got, G.expect(c, mode)))
