"""The reference's way to an aggregate, restated on (Tape, Strings.B, Message) arrays -- the checker of the device calls
sjhip_aggregate_path / sjhip_aggregate_path_records (test infrastructure, like where_walk.py, on rows_walk.RowWalk /
query_walk.Walk).

What a caller of the reference writes is a loop: FindElement(path...) and Iter.Int / Uint / Float on every row, the values that
converted added up and compared.  Here the column of that loop comes from column_walk.column -- values as 64-bit patterns and
statuses -- and is reduced in plain Python:

  reduce      one stretch of a column -> Agg: rows, the status histogram, count (the OK rows), not_ok, sum, min, max.  Integer sums
              are Python ints (exact); the float sum is math.fsum, the correctly rounded sum the device's association is held
              against; min and max go by key(): INT and UINT as integers, FLOAT by the total order of the doubles with -0.0 below
              +0.0 -- all bits of a negative value flipped, the sign bit of the others, compared unsigned.  Without an OK row: sum
              0, min and max None.
  column      the column of the rows of `w` (a RowWalk, or a Walk: its records); an empty path: the row's own value
  total       reduce over all rows
  per_record  reduce over the rows row_offsets[r] .. row_offsets[r + 1] of every record (rows_walk.select_rows' offsets, or
              where_walk.where's); None: no selection, record r owns row r
  record_arrays  per_record as the six arrays the device call fills (bit patterns; sum split into lo and hi of 128 bits)

AGG_TILE: the rows of one tile of the device's reduction (csrc/query.hip); the shapes of tests/test_gpu_aggregate.py come from it.
The geometry above one tile -- the two slots a tile hands on, the levels, the rows below a tile of a fold (32 768) and the
association of a float sum -- is restated in tests/agg_geometry.py; the shapes of tests/test_gpu_aggregate_seams.py come from that.
Pinned by tests/test_aggregate_walk.py."""
import math

import column_walk as CW

AGG_TILE = 256
U64 = (1 << 64) - 1
SIGN = 1 << 63


class Agg:
    def __init__(self, rows, status, total, lo, hi):
        self.rows, self.status, self.sum, self.min, self.max = rows, status, total, lo, hi
        self.count = status[CW.COL_OK]
        self.not_ok = rows - self.count

    def __repr__(self):
        return f"Agg(rows={self.rows}, status={self.status}, sum={self.sum!r}, min={self.min!r}, max={self.max!r})"


def key(bits, kind):
    """a uint64 whose unsigned order is the order of the kind"""
    if kind == CW.COL_UINT:
        return bits
    if kind == CW.COL_INT:
        return bits ^ SIGN
    return (~bits & U64) if bits >> 63 else bits ^ SIGN


def value(bits, kind):
    """the number a 64-bit pattern of the column stands for"""
    if kind == CW.COL_FLOAT:
        return CW.bits2f(bits)
    if kind == CW.COL_INT:
        return bits - (1 << 64) if bits >> 63 else bits
    return bits


def reduce(vals, sts, kind):
    status = [0] * 6
    for st in sts:
        status[st] += 1
    ok = [b for b, st in zip(vals, sts) if st == CW.COL_OK]
    if not ok:
        return Agg(len(sts), status, 0.0 if kind == CW.COL_FLOAT else 0, None, None)
    nums = [value(b, kind) for b in ok]
    total = math.fsum(nums) if kind == CW.COL_FLOAT else sum(nums)
    lo = value(min(ok, key=lambda b: key(b, kind)), kind)
    hi = value(max(ok, key=lambda b: key(b, kind)), kind)
    return Agg(len(sts), status, total, lo, hi)


def column(w, path, kind):
    if len(path):
        return CW.column(w, path, kind)
    vals, sts = [], []
    for root in w.records():  # (the row's own value: what FindElement of no keys stands on)
        st, x = CW.convert(w, root + 1, kind)
        vals.append(x)
        sts.append(st)
    return vals, sts


def total(w, path, kind):
    return reduce(*column(w, path, kind), kind)


def per_record(w, row_offsets, path, kind):
    vals, sts = column(w, path, kind)
    offs = list(range(len(vals) + 1)) if row_offsets is None else [int(o) for o in row_offsets]
    return [reduce(vals[a:b], sts[a:b], kind) for a, b in zip(offs[:-1], offs[1:])]


def bits_of(x, kind):
    """the 64-bit pattern of a min / max (None: 0)"""
    if x is None:
        return 0
    return CW.f2bits(x) if kind == CW.COL_FLOAT else x & U64


def record_arrays(aggs, kind):
    """-> (count, not_ok, sum lo, sum hi, min, max) as lists of uint64 patterns; a float sum: its bits in lo, hi 0"""
    out = ([], [], [], [], [], [])
    for a in aggs:
        s = CW.f2bits(a.sum) if kind == CW.COL_FLOAT else a.sum & ((1 << 128) - 1)
        for dst, x in zip(out, (a.count, a.not_ok, s & U64, s >> 64, bits_of(a.min, kind), bits_of(a.max, kind))):
            dst.append(x)
    return out
