"""The reference's way to a "group by", restated on (Tape, Strings.B, Message) arrays -- the checker of the device calls
sjhip_group_path / sjhip_fetch_groups / sjhip_fetch_group_aggregates (test infrastructure, like aggregate_walk.py, on
rows_walk.RowWalk / query_walk.Walk).

What a caller of the reference writes is a loop over the rows: FindElement(key path...) and Iter.StringBytes or Iter.Int, a map from
the key to a group that appends unseen keys to a slice, and per group the additions and comparisons of aggregate_walk.reduce on the
column at a second path.

  key_column   (keys, statuses) of the rows of `w`: bytes for STRING keys, the int64 for INT keys (None where the status is not OK);
               an empty path: the row's own value
  group        -> Grouping: keys in first-occurrence order, first_row, group_rows, codes (GROUP_NONE: no key), status, and -- with
               a value kind -- per group the aggregate_walk.Agg of the group's rows in row order
  arrays       the aggregates as the six arrays the device call fills (aggregate_walk.record_arrays)

GROUP_SORT_TILE (the rows of one tile of the device's sort by code, the largest tile of the new kernels), GROUP_RADIX_BITS (the
bits of a sort pass) and QTILE (the tile of the scans) come from csrc/sj_sort.h and csrc/sj_tapewalk.h; the shapes of
tests/test_gpu_group.py come from them.  Pinned by tests/test_group_walk.py.

The hash, the capacity and the probing of the device's key table are no part of this restatement (a dict stands in for them);
tests/group_table.py restates those, and builds the keys that put the table on its seams."""
import aggregate_walk as AW
import column_walk as CW

GROUP_NONE = 0xFFFFFFFF
GROUP_NO_VALUE = -1
COL_STRING = 4
GROUP_RADIX_BITS = 8
GROUP_SORT_THREADS, GROUP_SORT_ROUNDS = 256, 4
GROUP_SORT_TILE = GROUP_SORT_THREADS * GROUP_SORT_ROUNDS
QTILE = 1024


class Grouping:
    def __init__(self, rows, keys, first_row, group_rows, codes, status, aggs):
        self.rows, self.groups = rows, len(keys)
        self.keys, self.first_row, self.group_rows, self.codes, self.status, self.aggs = keys, first_row, group_rows, codes, status, aggs


def key_column(w, path, key_kind):
    keys, sts = [], []
    for root in w.records():
        v, st = (root + 1, CW.COL_OK) if len(path) == 0 else CW._at_path(w, root, path)
        k = None
        if v is not None:
            if key_kind == COL_STRING:
                st, b = CW.text(w, v, False)
                k = bytes(b) if st == CW.COL_OK else None
            elif key_kind == CW.COL_INT:
                st, x = CW.convert(w, v, CW.COL_INT)
                k = AW.value(x, CW.COL_INT) if st == CW.COL_OK else None
            else:
                raise ValueError(key_kind)
        keys.append(k)
        sts.append(st)
    return keys, sts


def group(w, key_path, key_kind, value_path=None, value_kind=None):
    keys, sts = key_column(w, key_path, key_kind)
    number, order, first_row, members, codes = {}, [], [], [], []
    for r, (k, st) in enumerate(zip(keys, sts)):
        if st != CW.COL_OK:
            codes.append(GROUP_NONE)
            continue
        g = number.get(k)
        if g is None:  # an unseen key is appended
            g = number[k] = len(order)
            order.append(k)
            first_row.append(r)
            members.append([])
        members[g].append(r)
        codes.append(g)
    aggs = None
    if value_kind is not None:
        vals, vsts = AW.column(w, () if value_path is None else value_path, value_kind)
        aggs = [AW.reduce([vals[r] for r in m], [vsts[r] for r in m], value_kind) for m in members]
    return Grouping(len(keys), order, first_row, [len(m) for m in members], codes, sts, aggs)


def arrays(g, value_kind):
    return AW.record_arrays(g.aggs, value_kind)
