"""GPU: the aggregates (sjhip_aggregate_path / sjhip_aggregate_path_records) against the serial restatement of
tests/aggregate_walk.py over the oracle's parse, and against the reduction of the device's own column (extract_path): on the
fixtures, on segment shapes built from the tile of the device's reduction (T = AGG_TILE rows: records that end on a wave edge, on a
tile edge and inside both, one that covers three whole tiles, runs of records without rows), on rows of every status, on integer
sums beyond 64 bits, on float sums (the bound that holds for every association, and the same bits from every call), under a row
predicate, through the error paths, and on a sharded result.

Counts, statuses, integer sums, min and max are compared bit for bit everywhere.  A float sum is compared bit for bit where every
partial sum of the values is exact (small integers and quarters: any association gives the same double), and otherwise against
math.fsum within (n - 1) u / (1 - (n - 1) u) * sum |x|, u = 2^-53: the error bound of recursive summation in ANY order of
the n - 1 additions (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2) -- the device's association is fixed but
is not the document order."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import aggregate_walk as AW
import column_walk as CW
import fixtures
import query_walk as Q
import rows_walk as RW
import where_walk as WW
import workloads
from test_aggregate_walk import STATUS_DOC, STATUS_WANT
from test_gpu_columns import oracle_walk
from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

F, I, U = CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT
KINDS = (F, I, U)
T = AW.AGG_TILE
ERR_ARG = 5
NAMES = ("count", "not_ok", "sum", "sum_hi", "min", "max")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def float_bound(vals, sts):
    """the bound of the module's docstring for the OK values of a stretch of a FLOAT column"""
    xs = [CW.bits2f(b) for b, st in zip(vals, sts) if st == CW.COL_OK]
    m = max(len(xs) - 1, 0) * 2.0 ** -53
    return m / (1 - m) * math.fsum(abs(x) for x in xs)


def same_total(got, want, kind, bound, what):
    print(what, "total:", got, "want:", want, "float bound:", bound)
    assert (got.rows, got.status, got.count) == (want.rows, want.status, want.count), what
    assert (got.min is None, got.max is None) == (want.min is None, want.max is None), what
    assert (AW.bits_of(got.min, kind), AW.bits_of(got.max, kind)) == (AW.bits_of(want.min, kind), AW.bits_of(want.max, kind)), what
    if kind != F:
        assert isinstance(got.sum, int) and got.sum == want.sum, what
    elif bound is None:
        assert CW.f2bits(got.sum) == CW.f2bits(want.sum), what
    else:
        assert abs(got.sum - want.sum) <= bound, (what, got.sum, want.sum, bound)
    raw = got.raw
    if want.count == 0:
        assert (raw.sum_lo, raw.sum_hi, raw.min, raw.max) == (0, 0, 0, 0), what
    if kind == F:
        assert raw.sum_hi == 0, what


def check_aggregates(ctx, rw, offsets, path, kind, exact=True, what=None):
    """aggregate_path and aggregate_path_records of the selection in force equal the checker; rw: a walk whose records() are the
    rows of that selection, offsets: its row offsets (None: no selection).  exact: the float sums are compared as bits."""
    what = (what, path, kind)
    vals, sts = AW.column(rw, path, kind)
    offs = list(range(len(vals) + 1)) if offsets is None else [int(o) for o in offsets]
    assert offs[-1] == len(vals), what
    total = ctx.aggregate_path(path, kind)
    same_total(total, AW.reduce(vals, sts, kind), kind, None if exact else float_bound(vals, sts), what)
    got = ctx.aggregate_path_records(path, kind)
    per = [AW.reduce(vals[a:b], sts[a:b], kind) for a, b in zip(offs[:-1], offs[1:])]
    want = AW.record_arrays(per, kind)
    dt = {F: np.float64, I: np.int64, U: np.uint64}[kind]
    assert [a.dtype for a in got] == [np.uint64, np.uint64, dt, np.uint64, dt, dt], what
    for j, name in enumerate(NAMES):
        assert len(got[j]) == len(per), (what, name)
        if name == "sum" and kind == F and not exact:
            for r, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
                assert abs(float(got[j][r]) - per[r].sum) <= float_bound(vals[a:b], sts[a:b]), (what, r)
            continue
        bad = np.flatnonzero(bits(got[j]) != np.array(want[j], dtype=np.uint64))
        assert len(bad) == 0, (what, name, bad[:5], bits(got[j])[bad[:5]], [want[j][k] for k in bad[:5]])
    assert int(got[0].sum()) == total.count and int(got[0].sum() + got[1].sum()) == total.rows, what
    return total, got


def check_device_column(ctx, offsets, path, kind, what):
    """... and the total and every record's entry are the reduction of the column the device extracts (offsets: the row offsets of
    the selection in force, None: record r owns row r)"""
    vals, st = ctx.extract_path(path, kind)
    vals, st = bits(vals).tolist(), st.tolist()
    what = (what, path, kind, "column")
    same_total(ctx.aggregate_path(path, kind), AW.reduce(vals, st, kind), kind, float_bound(vals, st), what)
    offs = list(range(len(vals) + 1)) if offsets is None else [int(o) for o in offsets]
    got = ctx.aggregate_path_records(path, kind)
    per = [AW.reduce(vals[a:b], st[a:b], kind) for a, b in zip(offs[:-1], offs[1:])]
    want = AW.record_arrays(per, kind)
    for j, name in enumerate(NAMES):
        if name == "sum" and kind == F:
            for r, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
                assert abs(float(got[j][r]) - per[r].sum) <= float_bound(vals[a:b], st[a:b]), (what, r)
        else:
            assert np.array_equal(bits(got[j]), np.array(want[j], dtype=np.uint64)), (what, name)


# ---- 1. equivalence with the column ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["twitter-statuses", "twitter-record", "parking-2000"])
def test_equals_the_reduced_column(ctx, case):
    if case == "parking-2000":
        doc = b"\n".join(workloads.c5_parking_nd(2).split(b"\n")[:2000])
        w = oracle_walk(doc, True, True)
        ctx.parse(doc, ndjson=True)
        rw, offs = w, None
        paths = [(b"Fine",), (b"Nope",)]  # (every member of this document is a string: a column of type errors)
        assert len(w.records()) == 2000
    else:
        doc = fixtures.load("twitter")
        w = oracle_walk(doc, False, True)
        ctx.parse(doc)
        if case == "twitter-statuses":
            offs, index, sts = RW.select_rows(w, (b"statuses",))
            assert ctx.select_rows((b"statuses",)) == (1, len(index))
            rw = RW.RowWalk(w, index)
            paths = [(b"retweet_count",), (b"user", b"followers_count"), (b"id",), (b"geo",), (b"user", b"name"), (b"user", b"id", b"x")]
        else:
            rw, offs = w, None
            paths = [(b"search_metadata", b"count"), (b"search_metadata", b"completed_in"), (b"statuses",)]
    for path in paths:
        for kind in KINDS:
            check_aggregates(ctx, rw, offs, path, kind, exact=False, what=case)
            check_device_column(ctx, offs, path, kind, case)
    ctx.select_records()


@pytest.mark.parametrize("n", [5, T + 3])
def test_records_without_a_selection(ctx, n):
    """record r owns one row, its root value: every record's entry is its own value or the identity, bit for bit"""
    texts = ["3", "-2.5", '"s"', "18446744073709551615", "-0.0", "null", "1e300", "-7", "0.25", "9223372036854775808.0"]
    lines = ['{"v":%s}' % texts[r % len(texts)] if r % 7 != 6 else '{"w":1}' for r in range(n)]
    doc = "\n".join(lines).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    for kind in KINDS:
        total, per = check_aggregates(ctx, w, None, (b"v",), kind, exact=False, what="records")
        check_device_column(ctx, None, (b"v",), kind, "records")
        assert total.rows == n and 1 < total.count < n and len(per[0]) == n
        ok = per[0] == 1
        vals, st = ctx.extract_path((b"v",), kind)
        assert np.array_equal(bits(per[2])[ok], bits(vals)[ok]) and np.array_equal(bits(per[4]), bits(per[5]))  # sum = min = max = the value
        assert np.array_equal(bits(per[4])[ok], bits(vals)[ok]) and not bits(per[4])[~ok].any()


# ---- 2. segment geometry -----------------------------------------------------------------------------------------------------------
def geometry_doc(name):
    """-> the rows of every record.  mixed: records that end on a wave edge (row 64), on a tile edge (row T), one that covers the
    three tiles behind it exactly, then sizes around the wave and the tile whose ends fall inside both; runs of records without rows
    at the start, in the middle and at the end"""
    if name == "one-record":
        return [3 * T + 5]
    if name == "one-row-each":
        return [1] * (2 * T + 3)
    return [0, 0, 0, 64, T - 64, 3 * T, 1, 63, 0, 0, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 0, 0]


@pytest.mark.parametrize("name", ["mixed", "one-record", "one-row-each"])
def test_segment_geometry(ctx, name):
    ks, lines, at = geometry_doc(name), [], 0
    for k in ks:  # small distinct integers of both signs: every float sum is exact
        lines.append('{"v":[%s]}' % ",".join(str((i + 1) * (-1 if i % 3 == 2 else 1)) for i in range(at, at + k)))
        at += k
    doc = "\n".join(lines).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    offs, index, sts = RW.select_rows(w, (b"v",))
    assert ctx.select_rows((b"v",)) == (len(ks), at) and offs == [sum(ks[:r]) for r in range(len(ks) + 1)]
    if name == "mixed":
        ends = set(offs)
        assert 64 in ends and T in ends and 4 * T in ends and any(e % 64 and e % T for e in ends)
    rw = RW.RowWalk(w, index)
    for kind in KINDS:
        total, per = check_aggregates(ctx, rw, offs, (), kind, exact=True, what=name)
        assert total.rows == at and (total.count == at if kind != U else 0 < total.count < at)
    ctx.select_records()


# ---- 3. every status ---------------------------------------------------------------------------------------------------------------
def test_every_status(ctx):
    w = oracle_walk(STATUS_DOC, False, True)
    ctx.parse(STATUS_DOC)
    offs, index, sts = RW.select_rows(w, (b"rows",))
    ctx.select_rows((b"rows",))
    rw = RW.RowWalk(w, index)
    for kind in KINDS:
        total, per = check_aggregates(ctx, rw, offs, (b"v",), kind, exact=False, what="statuses")
        hist, want_sum, lo, hi = STATUS_WANT[kind]
        assert total.status == hist and (total.min, total.max) == (lo, hi) and sum(hist) == total.rows
        if want_sum is not None:
            assert total.sum == want_sum  # only the OK rows
        check_device_column(ctx, offs, (b"v",), kind, "statuses")
    ctx.select_records()


def test_empty_path_histogram(ctx):
    scalars = ['"12"', "null", "true", "[1,2]", "-1", "9223372036854775808.0", "1e300", "18446744073709551616.0",
               "18446744073709551615", "3", "2.5", "{}"]
    doc = ('{"bare":[%s],"keyed":[%s]}' % (",".join(scalars), ",".join('{"v":%s}' % s for s in scalars))).encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    for kind in KINDS:
        offs, index, sts = RW.select_rows(w, (b"bare",))
        ctx.select_rows((b"bare",))
        bare, _ = check_aggregates(ctx, RW.RowWalk(w, index), offs, (), kind, exact=False, what="bare")
        offs, index, sts = RW.select_rows(w, (b"keyed",))
        ctx.select_rows((b"keyed",))
        keyed, _ = check_aggregates(ctx, RW.RowWalk(w, index), offs, (b"v",), kind, exact=False, what="keyed")
        assert bare.status == keyed.status and bytes(bare.raw) == bytes(keyed.raw) and bare.rows == len(scalars)
    ctx.select_records()


# ---- 4. exact integers ---------------------------------------------------------------------------------------------------------------
def test_integer_sums_beyond_64_bits(ctx):
    hi, lo, top = (1 << 63) - 1, -(1 << 63), (1 << 64) - 1
    records = [[hi] * 300, [lo] * 40 + [hi] * 10, [top] * 300]
    doc = "\n".join('{"v":[%s]}' % ",".join(map(str, r)) for r in records).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    offs, index, sts = RW.select_rows(w, (b"v",))
    ctx.select_rows((b"v",))
    rw = RW.RowWalk(w, index)
    total, per = check_aggregates(ctx, rw, offs, (), I, what="int")
    assert total.sum == 310 * hi + 40 * lo and total.raw.sum_hi != 0 and total.status[CW.COL_RANGE] == 300
    assert per[3].tolist() == [(300 * hi) >> 64, ((40 * lo + 10 * hi) >> 64) & top, 0] and per[3][0] != 0
    total, per = check_aggregates(ctx, rw, offs, (), U, what="uint")
    assert total.sum == 310 * hi + 300 * top and total.raw.sum_hi != 0 and total.status[CW.COL_RANGE] == 40
    assert per[3].tolist() == [(300 * hi) >> 64, (10 * hi) >> 64, (300 * top) >> 64] and per[3][2] == 299  # (the 40 negative rows: RANGE)
    ctx.select_records()


# ---- 5. the float sum: the bound of every association, the same bits from every call; the order of the zeros -------------------------
def test_float_sum_bound_and_determinism(ctx):
    rnd = random.Random(20251)
    n = 3 * T + 7
    xs = [rnd.choice((-1.0, 1.0)) * 10.0 ** rnd.uniform(-3, 12) for _ in range(n)]
    cut = T + 3  # two records, cut inside a tile: both carry a piece from one tile to the next
    doc = ('{"v":[%s]}\n{"v":[%s]}' % (",".join(map(repr, xs[:cut])), ",".join(map(repr, xs[cut:])))).encode()
    w = oracle_walk(doc, True, True)
    ctx.parse(doc, ndjson=True)
    offs, index, sts = RW.select_rows(w, (b"v",))
    assert ctx.select_rows((b"v",)) == (2, n)
    rw = RW.RowWalk(w, index)
    assert [CW.bits2f(b) for b in AW.column(rw, (), F)[0]] == xs  # the parse is exact
    total, per = check_aggregates(ctx, rw, offs, (), F, exact=False, what="float")
    u = 2.0 ** -53
    bound = (n - 1) * u / (1 - (n - 1) * u) * math.fsum(abs(x) for x in xs)
    print("float sum:", total.sum, "fsum:", math.fsum(xs), "difference:", total.sum - math.fsum(xs), "bound:", bound)
    assert abs(total.sum - math.fsum(xs)) <= bound
    again, per_again = ctx.aggregate_path((), F), ctx.aggregate_path_records((), F)
    assert bytes(again.raw) == bytes(total.raw)
    for a, b in zip(per, per_again):
        assert np.array_equal(bits(a), bits(b))
    ctx.select_records()


@pytest.mark.parametrize("rows", [["-0.0", "0.0", "-1.5", "2.5"], ["-0.0", "0.0"], ["0.0", "-0.0"], ["-0.0", "-0.0"]],
                         ids=["mixed", "zeros", "zeros-reversed", "negative-zeros"])
def test_float_min_max_order(ctx, rows):
    doc = ('{"v":[%s]}' % ",".join(rows)).encode()
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    offs, index, sts = RW.select_rows(w, (b"v",))
    ctx.select_rows((b"v",))
    total, per = check_aggregates(ctx, RW.RowWalk(w, index), offs, (), F, exact=(len(rows) == 4), what="zeros")
    if len(rows) == 4:
        assert (total.min, total.max, total.sum) == (-1.5, 2.5, 1.0)
    else:  # -0.0 ranks below +0.0, wherever it stands
        assert total.raw.min == 1 << 63 and total.raw.max == (1 << 63 if rows[0] == rows[1] else 0)
        assert total.raw.sum_lo == (1 << 63 if rows[0] == rows[1] else 0)  # IEEE: -0.0 + -0.0 = -0.0, -0.0 + 0.0 = +0.0
    ctx.select_records()


# ---- 6. under a row predicate --------------------------------------------------------------------------------------------------------
def test_under_where_path(ctx):
    doc = fixtures.load("twitter")
    w = oracle_walk(doc, False, True)
    ctx.parse(doc)
    base = RW.select_rows(w, (b"statuses",))
    name = (b"user", b"screen_name")

    def unchanged(sel, rw, records, nbytes):
        rows = len(sel[1])
        off, idx, st = ctx.fetch_rows(1, rows)
        assert off.tolist() == [0, rows] and idx.tolist() == sel[1] and st.tolist() == sel[2]
        o, data, s = ctx.fetch_path_strings(records, nbytes)
        want = RW.string_column(rw, name, False)
        assert o.tolist() == want[0] and bytes(data) == want[1] and s.tolist() == want[2]

    # twitter.json's statuses are 96 x "ja" and 4 x "zh"; two of their users have "en"
    for path, value, kept in [((b"lang",), b"zh", 4), ((b"user", b"lang"), b"en", 2)]:
        ctx.select_rows((b"statuses",))
        sel = WW.where(w, base, path, Q.OP_EQ_STRING, value)
        assert ctx.where_path(path, ctx.OP_EQ_STRING, value) == (1, kept) and len(sel[1]) == kept
        rw = RW.RowWalk(w, sel[1])
        records, nbytes = ctx.extract_path_strings(name, fetch=False)  # a product built beforehand
        for agg_path in [(b"retweet_count",), (b"user", b"followers_count")]:
            for kind in KINDS:
                check_aggregates(ctx, rw, sel[0], agg_path, kind, exact=False, what=(path, value))
        unchanged(sel, rw, records, nbytes)
    # lang == "en" keeps no row: rows 0, everything 0, every record the identity
    sel = WW.where(w, sel, (b"lang",), Q.OP_EQ_STRING, b"en")
    assert ctx.where_path((b"lang",), ctx.OP_EQ_STRING, b"en") == (1, 0) and sel[1] == []
    for kind in KINDS:
        a = ctx.aggregate_path((b"retweet_count",), kind)
        assert bytes(a.raw) == bytes(88) and (a.rows, a.count, a.sum, a.min, a.max) == (0, 0, 0, None, None)
        per = ctx.aggregate_path_records((b"retweet_count",), kind)
        assert all(len(x) == 1 and bits(x)[0] == 0 for x in per)
        check_aggregates(ctx, RW.RowWalk(w, []), sel[0], (b"retweet_count",), kind, what="no rows")
    o, data, s = ctx.fetch_path_strings(records, nbytes)  # the column of the two rows kept before is still there
    assert o.tolist() == RW.string_column(rw, name, False)[0]
    off, idx, st = ctx.fetch_rows(1, 0)
    assert off.tolist() == [0, 0] and len(idx) == 0 and st.tolist() == sel[2]
    ctx.select_records()


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_everything_alone(ctx):
    import sjhip
    L = sjhip.lib()
    doc = b'{"v":[1,2,3]}\n{"v":[4]}\n{"v":[]}'
    ctx.parse(doc, ndjson=True)
    assert ctx.select_rows((b"v",)) == (3, 4)
    before = ctx.fetch_rows(3, 4)
    lens, raw, n = (C.c_uint32 * 1)(1), sjhip._lib.Agg(), C.c_size_t(77)
    out = np.full(8, 7, dtype=np.uint64)
    for kind in (ctx.COL_BOOL, 4, 5, 99, -1):
        raw.rows = 123
        assert L.sjhip_aggregate_path(ctx._h, b"v", lens, 1, kind, C.byref(raw)) == ERR_ARG
        assert "kind %d" % kind in ctx.last_error() and raw.rows == 123, ctx.last_error()
        assert L.sjhip_aggregate_path_records(ctx._h, b"v", lens, 1, kind, out.ctypes.data, None, None, None, None, None, 8, C.byref(n)) == ERR_ARG
        assert "kind %d" % kind in ctx.last_error() and n.value == 77 and out.tolist() == [7] * 8, ctx.last_error()
    # too little room: the record count, and nothing written
    assert L.sjhip_aggregate_path_records(ctx._h, None, None, 0, I, out.ctypes.data, None, None, None, None, None, 2, C.byref(n)) == ERR_ARG
    assert n.value == 3 and out.tolist() == [7] * 8 and "room for 2 records" in ctx.last_error()
    with pytest.raises(sjhip.ParseError):
        ctx.aggregate_path((b"k",) * 17, I)  # a path longer than sjhip_find_path takes
    for a, b in zip(ctx.fetch_rows(3, 4), before):
        assert np.array_equal(a, b)
    assert ctx.aggregate_path((), I).sum == 10 and ctx.aggregate_path_records((), I)[2].tolist() == [6, 4, 0]
    assert L.sjhip_aggregate_path_records(ctx._h, None, None, 0, I, None, None, None, None, None, None, 3, C.byref(n)) == 0  # every destination null
    ctx.select_records()
    fresh = sjhip.Context(0)  # no result on the device
    assert L.sjhip_aggregate_path(fresh._h, b"v", lens, 1, I, C.byref(raw)) == ERR_ARG and fresh.last_error()
    assert L.sjhip_aggregate_path_records(fresh._h, b"v", lens, 1, I, None, None, None, None, None, None, 8, C.byref(n)) == ERR_ARG
    fresh.close()


# ---- 8. a sharded result ---------------------------------------------------------------------------------------------------------------
def test_sharded_result(ctx):
    import sjhip
    rnd = random.Random(8)
    pad = "x" * 230
    lines = []
    for r in range(11000):  # about 3 MB; quarters of small magnitude: every partial sum is exact, in any association
        nums = [repr(rnd.randrange(-4000, 4000) / 4) for _ in range(rnd.randrange(0, 6))]
        lines.append('{"pad":"%s","v":[%s]}' % (pad, ",".join(nums)))
    doc = "\n".join(lines).encode()
    assert len(doc) > 5 << 19
    many = sjhip.Context(0)
    try:
        with fixtures.nd_shard_limits(2 << 20, 1 << 20):
            many.parse(doc, ndjson=True)
        w = oracle_walk(doc, True, True)
        offs, index, sts = RW.select_rows(w, (b"v",))
        assert many.select_rows((b"v",)) == (len(lines), len(index))
        rw = RW.RowWalk(w, index)
        for kind in KINDS:
            check_aggregates(many, rw, offs, (), kind, exact=True, what="sharded rows")
        many.select_records()
        check_aggregates(many, w, None, (b"pad",), F, what="sharded records")  # no selection: a row per record, all type errors
    finally:
        many.close()
