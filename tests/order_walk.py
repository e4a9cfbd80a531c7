"""The reference's way to an "order by ... limit k", restated on (Tape, Strings.B, Message) arrays -- the checker of the device calls
sjhip_order_path / sjhip_fetch_order (test infrastructure, like group_walk.py, on rows_walk.RowWalk / query_walk.Walk).

What a caller of the reference writes is a loop over the rows -- FindElement(path...) and Iter.Float / Int / Uint --, a stable sort
of the row numbers by the converted value, and a slice of the first k.

  rank       the row numbers in rank order: Python's stable sorted() on (not ok, key), key = aggregate_walk.key -- the uint64 whose
             unsigned order is the order of the kind --, for a descending order the COMPLEMENT of the key, not the list reversed:
             equal keys stay in row order in both directions, and the rows without an OK key are last in both
  order      one call on the selection `sel` (row_offsets, row_index, statuses; None: no selection, record r owns its root value):
             key and status of every row from column_walk (aggregate_walk.column), the rank, the rows of rank < limit kept (0: all).
             The narrowing goes through where_walk.where's compaction -- the predicate "the row is kept" --, so every record keeps
             the kept rows it owned, in document order.  -> Ordering: records, rows, selection (row_offsets, row_index, statuses),
             order (the row number in the new selection of the row of rank i), values (bit patterns, 0 where not OK), status
  pass_mask  the digits (bytes) of the sort keys of the OK rows that differ at all: csrc/sj_sort.h order_pass_mask

ORDER_SORT_TILE (the rows of one tile of the device's sort, the largest tile of the new kernels), ORDER_RADIX_BITS (the bits of a
sort pass) and QTILE (the tile of the scans) come from csrc/sj_sort.h and csrc/sj_tapewalk.h; the shapes of tests/test_gpu_order.py
come from them.  Pinned by tests/test_order_walk.py and tests/test_order_abi.py."""
import aggregate_walk as AW
import column_walk as CW
import query_walk as Q
import rows_walk as RW
import where_walk as WW

ORDER_DESC = 1
ORDER_RADIX_BITS = 8
ORDER_SORT_THREADS, ORDER_SORT_ROUNDS = 256, 4
ORDER_SORT_TILE = ORDER_SORT_THREADS * ORDER_SORT_ROUNDS
QTILE = 1024
U64 = (1 << 64) - 1


class Ordering:
    def __init__(self, records, selection, order, values, status):
        self.records, self.rows, self.selection = records, len(order), selection
        self.order, self.values, self.status = order, values, status


def sort_key(bits, st, kind, descending):
    """what sorted() compares for one row"""
    if st != CW.COL_OK:
        return (True, 0)
    k = AW.key(bits, kind)
    return (False, ~k & U64 if descending else k)


def rank(vals, sts, kind, descending=False):
    return sorted(range(len(vals)), key=lambda r: sort_key(vals[r], sts[r], kind, descending))


class _Kept:
    """the walk where_walk.where asks: the element at tape index v "satisfies" iff it is the value of a kept row"""

    def __init__(self, w, kept):
        self.t, self.s, self.m, self.kept = w.t, w.s, w.m, kept

    def element_is(self, v, op, want=None):
        return v in self.kept


def order(w, sel, path, kind, descending=False, limit=0):
    offs, index, sts = WW.records_selection(w) if sel is None else sel
    index = [int(i) for i in index]
    vals, ksts = AW.column(RW.RowWalk(w, index), path, kind)
    ranked = rank(vals, ksts, kind, descending)
    n = len(ranked)
    kept = ranked if limit == 0 or limit >= n else ranked[:limit]
    selection = WW.where(_Kept(w, {index[r] for r in kept}), (offs, index, sts), (), Q.OP_EXISTS)
    number = {old: new for new, old in enumerate(sorted(kept))}  # the row numbers of the new selection
    return Ordering(len(offs) - 1, selection, [number[r] for r in kept], [vals[r] for r in kept], [ksts[r] for r in kept])


def pass_mask(vals, sts, kind, descending=False):
    keys = [sort_key(b, st, kind, descending)[1] for b, st in zip(vals, sts) if st == CW.COL_OK]
    if len(keys) < 2:
        return 0
    all_, any_ = U64, 0
    for k in keys:
        all_ &= k
        any_ |= k
    varying = all_ ^ any_
    return sum(1 << p for p in range(8) if (varying >> (ORDER_RADIX_BITS * p)) & 0xFF)
