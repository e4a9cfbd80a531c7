"""CPU: tests/agg_geometry.py agrees with the source text of csrc/query.hip and with aggregate_walk.reduce, every case of its lists
lies on the cut its claim names (read from the model's trace), the float cases tell the device's association from the document
order and from the correctly rounded sum, and the case lists tell six deliberately wrong reductions from the right one -- the
condition that keeps tests/test_gpu_aggregate_seams.py from being vacuous.  No case list may be thinned until a mutant survives."""
import functools
import math
import os
import random
import re

import aggregate_walk as AW
import agg_geometry as G
import column_walk as CW

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simdjson-go_amd", "csrc")
F, I, U = G.FLOAT, G.INT, G.UINT
T, FT = G.T, G.F


def want_arrays(vals, sts, offs, kind):
    return AW.record_arrays([AW.reduce(vals[a:b], sts[a:b], kind) for a, b in zip(offs[:-1], offs[1:])], kind)


@functools.lru_cache(maxsize=None)
def model(case, kind, mutant=None):
    """-> (per-record arrays, their trace, the total's arrays, its trace)"""
    vals, sts = G.column(case, kind)
    per, trace = G.run(vals, sts, None if case.own else G.offsets(case), kind, mutant=mutant)
    total, ttrace = G.run(vals, sts, None, kind, one_segment=True, mutant=mutant)
    return per, trace, total, ttrace


# ---- the constants against the source -----------------------------------------------------------------------------------------------
def test_mirror_constants_are_the_sources():
    src = open(os.path.join(CSRC, "query.hip")).read()
    assert int(re.search(r"static constexpr int AGG_TILE = (\d+);", src).group(1)) == G.AGG_TILE == AW.AGG_TILE
    # agg_layout: AGG_TILE items per tile, two items per tile to the next level, until a level is one tile
    layout = src[src.index("static size_t agg_layout("):src.index("static int agg_enqueue(")]
    assert re.search(r"const u32 tiles = \(m \+ AGG_TILE - 1\) / AGG_TILE;", layout)
    assert re.search(r"if \(tiles == 1\) break;\s+m = 2 \* tiles;", layout)
    assert len(re.findall(r"a\.items\[2ull \* blockIdx\.x( \+ 1)?\]", src)) == 3  # slots A (twice: the item, or none) and B
    assert re.search(r"enum : u32 \{ AGG_VALID = 1, AGG_HEAD = 2, AGG_END = 4 \};", src) and (G.VALID, G.HEAD, G.END) == (1, 2, 4)
    assert re.search(r"const u32 m = 2 \* w\.tiles\[l - 1\];", src)
    assert G.ROWS_PER_FOLD_TILE == G.AGG_TILE * G.AGG_TILE // 2 == 32768 and G.ROWS_PER_FOLD2_TILE == 128 * 32768
    for n, want in [(1, [1]), (256, [1]), (257, [2, 1]), (FT, [128, 1]), (FT + 1, [129, 2, 1]), (G.ROWS_PER_FOLD2_TILE, [16384, 128, 1]),
                    (G.ROWS_PER_FOLD2_TILE + 1, [16385, 129, 2, 1]), (1000000, [3907, 31, 1])]:
        assert G.levels(n) == want, n


# ---- the model against the plain reduction ------------------------------------------------------------------------------------------
def random_column(rnd, n, kind):
    """values whose sums are exact in any association: quarters (FLOAT), integers up to the ends of the kind (INT / UINT)"""
    vals, sts = [], []
    big = rnd.random() < 0.3
    for _ in range(n):
        if rnd.random() < 0.15:
            vals.append(0)
            sts.append(rnd.choice((CW.COL_NOT_FOUND, CW.COL_TYPE, CW.COL_NULL, CW.COL_RANGE)))
            continue
        if kind == F:
            x = CW.f2bits(rnd.randrange(-4000, 4000) / 4)  # (-0.0: the floats list; math.fsum does not keep its sign)
        elif kind == I:
            x = (rnd.choice((-(1 << 63), (1 << 63) - 1, -1, 1 << 32, -(1 << 32) - 1)) if big else rnd.randrange(-1000, 1000)) & G.U64
        else:
            x = rnd.choice((G.U64, 1 << 63, (1 << 32) - 1, 1 << 32)) if big else rnd.randrange(0, 2000)
        vals.append(x)
        sts.append(CW.COL_OK)
    return vals, sts


def random_offsets(rnd, n):
    style = rnd.randrange(4)
    if style == 0:
        cuts = []
    elif style == 1:
        cuts = [rnd.randrange(n + 1) for _ in range(rnd.randrange(1, 4))]
    elif style == 2:  # many short records and runs of records without rows
        cuts = [rnd.randrange(n + 1) for _ in range(rnd.randrange(n // 3 + 1, n + 2))]
    else:  # on the edges of waves and tiles
        cuts = [min(n, k * 64 + rnd.choice((-1, 0, 0, 1))) for k in range(1, n // 64 + 1) if rnd.random() < 0.5]
    return [0] + sorted(max(c, 0) for c in cuts) + [n]


def check_against_reduce(rnd, n, kind, own=True):
    vals, sts = random_column(rnd, n, kind)
    offs = random_offsets(rnd, n)
    got, trace = G.run(vals, sts, offs, kind)
    assert tuple(map(list, got)) == tuple(map(list, want_arrays(vals, sts, offs, kind))), (n, kind, offs[:8])
    assert trace.tiles == G.levels(n) and len(trace.items) == len(trace.tiles) and trace.items[-1] == []
    one, _ = G.run(vals, sts, None, kind, one_segment=True)
    assert tuple(map(list, one)) == tuple(map(list, want_arrays(vals, sts, [0, n], kind))), (n, kind)
    if not own:
        return
    own, _ = G.run(vals, sts, None, kind)
    assert tuple(map(list, own)) == tuple(map(list, want_arrays(vals, sts, list(range(n + 1)), kind))), (n, kind)


def test_model_equals_the_plain_reduction():
    rnd = random.Random(7)
    sizes = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T, 3 * T] + [rnd.randrange(1, 3 * T + 1) for _ in range(290)]
    for k, n in enumerate(sizes):
        check_against_reduce(rnd, n, (F, I, U)[k % 3])
    assert G.run([], [], [0, 0, 0], I)[0] == tuple([0, 0] for _ in range(6))  # no rows: nothing runs, the outputs stay 0


def test_model_equals_the_plain_reduction_around_the_fold_tile():
    rnd = random.Random(8)
    sizes = [FT - T, FT, FT + 1, 2 * FT, 2 * FT + 1, 2 * FT + T] + [rnd.randrange(FT - T, 2 * FT + T + 1) for _ in range(6)]
    for k, n in enumerate(sizes):
        check_against_reduce(rnd, n, (F, I, U)[k % 3], own=False)


# ---- every case on its cut ----------------------------------------------------------------------------------------------------------
def test_every_case_lies_on_its_cut():
    seen, by_levels = set(), {}
    for name, cases in (("level_counts", G.level_counts()), ("fold_seams", G.fold_seams()), ("statuses", G.statuses()), ("floats", G.floats())):
        assert len({c.name for c in cases}) == len(cases)
        for c in cases:
            kind = F if name == "floats" else I
            per, trace, total, ttrace = model(c, kind)
            seen.update(G.holds(c, ttrace if c.own else trace, None if c.own else per))
            assert ttrace.tiles == G.levels(sum(c.rows)) and ttrace.stored == {0: len(ttrace.tiles) - 1}  # the total: the last level
            by_levels.setdefault(name, []).append(len(ttrace.tiles))
            vals, sts = G.column(c, kind)
            if name != "floats":  # integers: the model is the plain reduction
                assert tuple(map(list, per)) == tuple(map(list, want_arrays(vals, sts, list(range(len(vals) + 1)) if c.own else G.offsets(c), kind)))
                assert tuple(map(list, total)) == tuple(map(list, want_arrays(vals, sts, [0, len(vals)], kind)))
    assert seen >= {"levels", "stored", "tiles", "cut", "b_at_255", "a_end_first_slot", "a_open_first_slot", "a_open_whole_tile",
                    "b_from_invalid_last", "second_fold_ab", "head_in_wave", "empty_at", "heads_at", "all_at_level", "no_items", "bad_tile", "all_zero", "own"}
    assert sorted(set(by_levels["level_counts"])) == [1, 2, 3] and set(by_levels["fold_seams"]) == {3} and set(by_levels["floats"]) == {3}
    # the seams of level_counts: both sides of 256 | 257 and of F | F + 1, as one record and (the small ones) as one-row records
    rows = sorted(sum(c.rows) for c in G.level_counts() if not c.own)
    assert rows == [1, 63, 64, 65, 255, 256, 257, FT - 1, FT, FT + 1, FT + 255, FT + 256, FT + 257]
    assert sorted(sum(c.rows) for c in G.level_counts() if c.own) == rows[:7]
    assert {c.claim["cut"] - FT for c in G.fold_seams() if "cut" in c.claim} == {-T, -1, 0, 1, T}
    four, = G.four_levels()
    assert len(G.levels(sum(four.rows))) == 4 == four.claim["levels"] and len(G.levels(four.rows[0] + 3)) == 3
    d = G.digits(sum(four.rows))
    assert int(d.min()) == -9 and int(d.max()) == 9 and len(set(d[:100].tolist())) > 10


def test_status_cases_reach_every_kind():
    for c in G.statuses():
        for kind in (F, I, U):
            sts = G.column(c, kind)[1]
            assert 0 < sts.count(CW.COL_OK) < len(sts) or "without" in c.name


# ---- the float cases --------------------------------------------------------------------------------------------------------------
def test_float_cases_have_teeth():
    u = 2.0 ** -53
    for c in G.floats():
        per, trace, total, ttrace = model(c, F)
        vals, sts = G.column(c, F)
        assert set(sts) == {CW.COL_OK}
        xs = [CW.bits2f(b) for b in vals]
        offs = G.offsets(c)
        stretches = list(zip(offs[:-1], offs[1:]))
        if "teeth" in c.claim:
            assert all(math.isfinite(x) and abs(x) >= 2.0 ** -1022 for x in xs) and [repr(x) for x in xs] == G.texts(c)
            differs_ltr = differs_fsum = 0
            for r, (a, b) in enumerate(stretches + [(0, len(xs))]):
                got = CW.bits2f((per[2][r] if r < len(stretches) else total[2][0]))
                ltr = 0.0
                for x in xs[a:b]:
                    ltr += x
                exact = math.fsum(xs[a:b])
                differs_ltr += got != ltr
                differs_fsum += got != exact
                m = (b - a - 1) * u
                bound = m / (1 - m) * math.fsum(abs(x) for x in xs[a:b])
                assert abs(got - exact) <= bound, (c.name, r, got, exact, bound)
            assert differs_ltr and differs_fsum, (c.name, differs_ltr, differs_fsum)
        else:  # the zeros: -0.0 through every identity, empty slot and fold; one +0.0 in the last row turns its record and the total
            want = [c.claim["sum_bits"]] * len(stretches)
            if "last_sum_bits" in c.claim:
                want[-1] = c.claim["last_sum_bits"]
            assert list(per[2]) == want and total[2][0] == want[-1], (c.name, per[2], total[2])
            assert all(b in (0, 1 << 63) for b in vals) and (vals[-1] == 0) == ("last_sum_bits" in c.claim)


# ---- mutants ------------------------------------------------------------------------------------------------------------------------
def test_join_is_commutative_so_the_swap_that_counts_is_the_one_of_the_roles():
    """agg_join(o, v) and agg_join(v, o) are the same function: IEEE addition, integer addition, min and max all commute.  The mutant
    "o and v swapped" therefore swaps the ROLES in the scan step -- the lane in front is taken for the one behind, so that ITS head
    stops the join --; the plain swap of the arguments is no mistake any test could see, which this pins."""
    rnd = random.Random(3)
    for kind in (F, I, U):
        for _ in range(500):
            a, b = (G.row_value(rnd.getrandbits(64) if kind != F else CW.f2bits(rnd.uniform(-1e12, 1e12)), CW.COL_OK, kind) for _ in range(2))
            assert G.join(a, b, kind) == G.join(b, a, kind)
    z = G.join(G.row_value(1 << 63, 0, F), G.row_value(0, 0, F), F), G.join(G.row_value(0, 0, F), G.row_value(1 << 63, 0, F), F)
    assert [CW.f2bits(x[2]) for x in z] == [0, 0]


def test_case_lists_catch_every_mutant():
    lists = [("fold_seams", G.fold_seams(), (I,)), ("statuses", G.statuses(), (I,)), ("floats", G.floats(), (F,))]
    caught = {}
    for mutant in G.MUTANTS:
        for name, cases, kinds in lists:
            for c in cases:
                for kind in kinds:
                    if mutant == "identity +0.0" and kind != F:
                        continue  # (the integer identity is 0 either way: the mutant is the reduction itself there)
                    right = model(c, kind)
                    vals, sts = G.column(c, kind)
                    per, _ = G.run(vals, sts, None if c.own else G.offsets(c), kind, mutant=mutant)
                    total, _ = G.run(vals, sts, None, kind, one_segment=True, mutant=mutant)
                    if (per, total) != (right[0], right[2]):
                        caught.setdefault(mutant, "%s: %s" % (name, c.name))
                        break
                if mutant in caught:
                    break
            if mutant in caught:
                break
        assert mutant in caught, "no case of fold_seams, statuses or floats tells the mutant %r from the reduction" % mutant
    print(caught)
    assert len(caught) == len(G.MUTANTS) == 6, "first catches: %r" % caught
    # the zeros are the only cases that can see the identity; the rest are seen where segments cross tiles
    assert caught["identity +0.0"].startswith("floats: ") and "-0.0" in caught["identity +0.0"], caught
