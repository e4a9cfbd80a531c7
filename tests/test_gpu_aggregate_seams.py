"""GPU: the segmented reduction under sjhip_aggregate_path, sjhip_aggregate_path_records and the aggregates of sjhip_group_path(s)
on the seams tests/agg_geometry.py names -- the 256 | 257-row and the 32 768 | 32 769-row seams between one, two and three levels,
the cuts of a record around a tile of level 1 (a B item at index 255, an A item in the first slot of the next tile, a slot A
open over a whole tile, a second fold that reads A and B items), records without rows, rows that are not OK, and four levels.

Every case of level_counts, fold_seams and statuses, for FLOAT, INT and UINT, is compared bit for bit with the host model
(agg_geometry.run) and with aggregate_walk.reduce over the oracle's parse (check_aggregates of tests/test_gpu_aggregate.py): the
values are small integers of both signs, so every association gives the same double.  The floats cases hold the sum of every
record and of the total to the BITS of the model -- the device's association, restated -- and to the bound of every association
around math.fsum.  tests/test_agg_geometry.py proves on the CPU that these lists tell six wrong reductions from the right one."""
import functools
import math

import numpy as np
import pytest

import aggregate_walk as AW
import agg_geometry as G
import column_walk as CW
import fixtures
import group_walk as GW
import query_walk as Q
import rows_walk as RW
import where_walk as WW
from test_gpu_aggregate import bits, check_aggregates, float_bound
from test_gpu_columns import oracle_walk
from test_gpu_group import check_group
from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

F, I, U, S = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT, GW.COL_STRING
KINDS = (F, I, U)
T, FT = G.T, G.F
CASES = {name: {c.name: c for c in cases()} for name, cases in
         (("level_counts", G.level_counts), ("fold_seams", G.fold_seams), ("statuses", G.statuses), ("floats", G.floats))}


@functools.lru_cache(maxsize=2)
def walked(case):
    """the document, its rows as a walk of the oracle's parse and their offsets (None: no selection), once per case"""
    doc = G.doc(case)
    w = oracle_walk(doc, True, True)
    if case.own:
        assert len(w.records()) == len(case.rows)
        return doc, w, None
    offs, index, sts = RW.select_rows(w, (b"v",))
    assert offs == G.offsets(case)
    return doc, RW.RowWalk(w, index), offs


@functools.lru_cache(maxsize=6)
def column(case, kind):
    doc, rw, offs = walked(case)
    vals, sts = AW.column(rw, (b"v",) if case.own else (), kind)
    assert (vals, sts) == G.column(case, kind)  # the generator's column is the oracle's
    return vals, sts


def load(ctx, case):
    doc, rw, offs = walked(case)
    ctx.parse(doc, ndjson=True)
    if not case.own:
        assert ctx.select_rows((b"v",)) == (len(case.rows), sum(case.rows))
    return rw, offs, ((b"v",) if case.own else ())


def same_as_the_model(case, kind, total, per):
    """the device's arrays and its total are the model's, bit for bit -> the model's arrays (per record, total)"""
    vals, sts = column(case, kind)
    want, trace = G.run(vals, sts, None if case.own else G.offsets(case), kind)
    for j, name in enumerate(("count", "not_ok", "sum", "sum_hi", "min", "max")):
        bad = np.flatnonzero(bits(per[j]) != np.array(want[j], dtype=np.uint64))
        assert len(bad) == 0, (case.name, kind, name, bad[:5], bits(per[j])[bad[:5]], [want[j][k] for k in bad[:5]])
    one, ttrace = G.run(vals, sts, None, kind, one_segment=True)
    raw = total.raw
    got = (total.count, total.rows - total.count, int(raw.sum_lo), int(raw.sum_hi), int(raw.min), int(raw.max))
    assert got == tuple(col[0] for col in one), (case.name, kind, got, one)
    assert len(ttrace.tiles) == case.claim["levels"]
    return want, one


def run_case(ctx, case, kind):
    rw, offs, path = load(ctx, case)
    total, per = check_aggregates(ctx, rw, offs, path, kind, exact=True, what=case.name)
    same_as_the_model(case, kind, total, per)
    assert total.rows == sum(case.rows) and len(per[0]) == len(case.rows)
    if not case.own:
        ctx.select_records()


@pytest.mark.parametrize("kind", KINDS, ids=["float", "int", "uint"])
@pytest.mark.parametrize("name", list(CASES["level_counts"]))
def test_level_counts(ctx, name, kind):
    run_case(ctx, CASES["level_counts"][name], kind)


@pytest.mark.parametrize("kind", KINDS, ids=["float", "int", "uint"])
@pytest.mark.parametrize("name", list(CASES["fold_seams"]))
def test_fold_seams(ctx, name, kind):
    run_case(ctx, CASES["fold_seams"][name], kind)


@pytest.mark.parametrize("kind", KINDS, ids=["float", "int", "uint"])
@pytest.mark.parametrize("name", list(CASES["statuses"]))
def test_statuses(ctx, name, kind):
    case = CASES["statuses"][name]
    run_case(ctx, case, kind)
    if "all_zero" in case.claim:
        r = case.claim["all_zero"]
        rw, offs, path = load(ctx, case)
        per = ctx.aggregate_path_records(path, kind)
        assert int(per[1][r]) == case.rows[r] and all(int(bits(per[j])[r]) == 0 for j in (0, 2, 3, 4, 5))
        ctx.select_records()


@pytest.mark.parametrize("name", list(CASES["floats"]))
def test_floats(ctx, name):
    """the sums as bits of the model and inside the bound of every association; the same bytes from a second call"""
    case = CASES["floats"][name]
    rw, offs, path = load(ctx, case)
    total, per = check_aggregates(ctx, rw, offs, path, F, exact=False, what=name)  # count, min, max, the histogram; sums: the bound
    vals, sts = column(case, F)
    xs = [CW.bits2f(b) for b in vals]
    want, one = same_as_the_model(case, F, total, per)
    for r, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        bound = float_bound(vals[a:b], sts[a:b])
        print(name, "record", r, "sum:", float(per[2][r]), "fsum:", math.fsum(xs[a:b]), "bound:", bound)
        assert abs(float(per[2][r]) - math.fsum(xs[a:b])) <= bound
    bound = float_bound(vals, sts)
    print(name, "total:", total.sum, "fsum:", math.fsum(xs), "bound:", bound)
    assert abs(total.sum - math.fsum(xs)) <= bound
    if "sum_bits" in case.claim:
        sums = [case.claim["sum_bits"]] * (len(offs) - 2) + [case.claim.get("last_sum_bits", case.claim["sum_bits"])]
        assert bits(per[2]).tolist() == sums and int(total.raw.sum_lo) == sums[-1]
    again, per_again = ctx.aggregate_path(path, F), ctx.aggregate_path_records(path, F)
    assert bytes(again.raw) == bytes(total.raw)
    for a, b in zip(per, per_again):
        assert np.array_equal(bits(a), bits(b))
    ctx.select_records()


def test_four_levels(ctx):
    """4 194 561 rows: a third fold.  The expectation is integer arithmetic on the generator's own values"""
    case, = G.four_levels()
    n = sum(case.rows)
    assert len(G.levels(n)) == 4 and len(G.levels(case.rows[0])) == 3
    d = G.digits(n)
    cut = case.rows[0]
    ctx.parse(G.doc(case), ndjson=True)
    assert ctx.select_rows((b"v",)) == (2, n)
    starts = np.array([0, cut])
    for kind in KINDS:
        ok = d >= 0 if kind == U else np.ones(n, dtype=bool)
        x = np.where(ok, d, 0)
        total, per = ctx.aggregate_path((), kind), ctx.aggregate_path_records((), kind)
        assert (total.rows, total.count, total.status[CW.COL_RANGE]) == (n, int(ok.sum()), n - int(ok.sum()))
        assert total.sum == int(x.sum()) and total.min == (0 if kind == U else -9) and total.max == 9
        assert per[0].tolist() == np.add.reduceat(ok.astype(np.int64), starts).tolist()
        assert per[1].tolist() == np.add.reduceat((~ok).astype(np.int64), starts).tolist()
        assert per[2].astype(np.float64).tolist() == np.add.reduceat(x, starts).astype(np.float64).tolist()
        assert bits(per[3]).tolist() == [(int(s) >> 64) & G.U64 if kind != F else 0 for s in np.add.reduceat(x, starts)]
        assert per[4].tolist() == [0 if kind == U else -9] * 2 and per[5].tolist() == [9, 9]
    ctx.select_records()


# ---- groups: the same reduction over the rows ordered by group -------------------------------------------------------------------------
def group_lines(shape):
    if shape == "one group":
        keys = ["g"] * (FT + T + 3)
    elif shape == "three keys interleaved":
        left, keys = {"a": FT + 1, "b": T, "c": 5}, []
        while left:
            for k in list(left):
                keys.append(k)
                left[k] -= 1
                if not left[k]:
                    del left[k]
    else:  # the rows r = 0 (mod 3) have the key, the others none
        keys = ["g" if r % 3 == 0 else None for r in range(3 * FT + 9)]
    vals = [(r % 1999 + 1) * (-1 if r % 3 == 2 else 1) for r in range(len(keys))]
    return ['{"v":%d}' % v if k is None else '{"k":"%s","v":%d}' % (k, v) for k, v in zip(keys, vals)]


@functools.lru_cache(maxsize=1)
def group_walked(shape):
    doc = "\n".join(group_lines(shape)).encode()
    return doc, oracle_walk(doc, True, True)


@pytest.mark.parametrize("kind", [I, F], ids=["int", "float"])
@pytest.mark.parametrize("shape", ["one group", "three keys interleaved", "every third row"])
def test_groups_over_a_fold_tile(ctx, shape, kind):
    doc, w = group_walked(shape)
    ctx.parse(doc, ndjson=True)
    got, want = check_group(ctx, w, (b"k",), S, (b"v",), kind, what=shape)
    assert len(G.levels(int(got.group_rows.sum()))) == 3 and int(got.group_rows.max()) > FT
    if shape == "three keys interleaved":  # the order inside a group is the row order
        assert got.group_rows.tolist() == [FT + 1, T, 5] and got.first_row.tolist() == [0, 1, 2]
    elif shape == "every third row":
        assert got.group_rows.tolist() == [FT + 3] and got.rows == 3 * FT + 9
    else:
        assert got.group_rows.tolist() == [FT + T + 3]
        if kind == I:  # one group_paths call, two aggregates from the same grouping
            both = ctx.group_paths([((b"k",), S)], [((b"v",), I), ((b"v",), F)])
            assert (both.rows, both.groups) == (got.rows, 1) and both.group_rows.tolist() == got.group_rows.tolist()
            flt = ctx.group_path((b"k",), S, (b"v",), F)
            for mine, theirs in ((both.values[0], got.aggregates()), (both.values[1], flt.aggregates())):
                for a, b in zip(mine, theirs):
                    assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---- under a row predicate that keeps every second row, whole and sharded --------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def where_walked():
    case = CASES["fold_seams"][G.THREE]
    at, lines = 0, []
    for k in case.rows:  # twice the rows of the three-fold-tile shape; the rows with "a":0 are that shape
        lines.append('{"v":[%s]}' % ",".join('{"a":%d,"x":%d}' % (i % 2, (i // 2 + 1) * (-1 if i % 3 == 2 else 1)) for i in range(at, at + 2 * k)))
        at += 2 * k
    doc = "\n".join(lines).encode()
    w = oracle_walk(doc, True, True)
    base = RW.select_rows(w, (b"v",))
    sel = WW.where(w, base, (b"a",), Q.OP_EQ_INT, 0)
    assert sel[0] == G.offsets(case) and len(base[1]) == 2 * len(sel[1])
    return doc, w, sel


@pytest.mark.parametrize("sharded", [False, True], ids=["whole", "sharded"])
def test_three_fold_tiles_under_where_path(ctx, sharded):
    import sjhip
    doc, w, sel = where_walked()
    rows = sel[0][-1]
    c = sjhip.Context(0) if sharded else ctx
    try:
        if sharded:  # a record is never cut: the shard that owns record 1 owns its F + 3 T + 16 rows
            assert len(doc) > 2 << 20 and sel[0][2] - sel[0][1] > FT
            with fixtures.nd_shard_limits(2 << 20, 2 << 20):
                c.parse(doc, ndjson=True)
        else:
            c.parse(doc, ndjson=True)
        assert c.select_rows((b"v",)) == (3, 2 * rows)
        assert c.where_path((b"a",), c.OP_EQ_INT, 0) == (3, rows)
        rw = RW.RowWalk(w, sel[1])
        for kind in KINDS:
            total, per = check_aggregates(c, rw, sel[0], (b"x",), kind, exact=True, what=("where", sharded))
            assert total.rows == rows and len(G.levels(rows)) == 3
        c.select_records()
    finally:
        if sharded:
            c.close()
