"""The "group by" of several keys with several aggregates, restated on (Tape, Strings.B, Message) arrays -- the checker of the device
calls sjhip_group_paths / sjhip_fetch_group_keys / sjhip_fetch_group_aggregates_at (test infrastructure, like group_walk.py, on
rows_walk.RowWalk / query_walk.Walk, column_walk and aggregate_walk).

What a caller of the reference writes is group_walk's loop with a tuple as the map's key: per key column FindElement(path...) and
Iter.StringBytes / Int / Uint / Bool; an entry of the tuple is (True, key) where the column's status is OK and NO_KEY = (False, None)
where it is not and the column carries the null-key flag; a row with a column that is not OK and has no flag is in no group.  A dict
of tuples numbers the groups by first occurrence.

  key_column   (keys, statuses) of one column of the rows of `w`: bytes for STRING, the number for INT / UINT, 0 / 1 for BOOL
  group        key_columns = [(path, kind) or (path, kind, null_key)], value_columns = [(path, kind)] -> MultiGrouping: per
               column keys (the group's entry: the key, or None for "no key"), key_ok and status (every row's, whatever the other
               columns give); first_row, group_rows, codes; aggs[v]: per group the aggregate_walk.Agg of the group's rows in row order
  key_bytes    what sjhip_group_paths reports per column
Pinned by tests/test_group_multi_walk.py.  The hash of a tuple and the table are no part of this: tests/group_multi_table.py."""
import aggregate_walk as AW
import column_walk as CW
import group_walk as GW

GROUP_NONE, COL_STRING = GW.GROUP_NONE, GW.COL_STRING
GROUP_MAX_KEYS, GROUP_MAX_VALUES, GROUP_NULL_KEY = 8, 8, 1
KEY_KINDS = (COL_STRING, CW.COL_INT, CW.COL_UINT, CW.COL_BOOL)
NO_KEY = (False, None)


class MultiGrouping:
    def __init__(self, rows, keys, key_ok, status, first_row, group_rows, codes, aggs):
        self.rows, self.groups = rows, len(first_row)
        self.keys, self.key_ok, self.status = keys, key_ok, status
        self.first_row, self.group_rows, self.codes, self.aggs = first_row, group_rows, codes, aggs


def key_column(w, path, kind):
    if kind in (COL_STRING, CW.COL_INT):
        return GW.key_column(w, path, kind)
    if kind not in KEY_KINDS:
        raise ValueError(kind)
    keys, sts = [], []
    for root in w.records():
        v, st = (root + 1, CW.COL_OK) if len(path) == 0 else CW._at_path(w, root, path)
        k = None
        if v is not None:
            st, x = CW.convert(w, v, kind)
            k = x if st == CW.COL_OK else None
        keys.append(k)
        sts.append(st)
    return keys, sts


def group(w, key_columns, value_columns=()):
    cols = [(tuple(c[0]), c[1], bool(c[2]) if len(c) > 2 else False) for c in key_columns]
    if not 1 <= len(cols) <= GROUP_MAX_KEYS or len(value_columns) > GROUP_MAX_VALUES:
        raise ValueError((len(cols), len(value_columns)))
    columns = [key_column(w, path, kind) for path, kind, _ in cols]
    n = len(columns[0][0])
    number, tuples, first_row, members, codes = {}, [], [], [], []
    for r in range(n):
        entries = []
        for (keys, sts), (_, _, null_key) in zip(columns, cols):
            if sts[r] == CW.COL_OK:
                entries.append((True, keys[r]))
            elif null_key:
                entries.append(NO_KEY)
            else:
                entries = None
                break
        if entries is None:
            codes.append(GROUP_NONE)
            continue
        t = tuple(entries)
        g = number.get(t)
        if g is None:  # an unseen tuple is appended
            g = number[t] = len(tuples)
            tuples.append(t)
            first_row.append(r)
            members.append([])
        members[g].append(r)
        codes.append(g)
    aggs = []
    for path, kind in value_columns:
        vals, vsts = AW.column(w, tuple(path), kind)
        aggs.append([AW.reduce([vals[r] for r in m], [vsts[r] for r in m], kind) for m in members])
    return MultiGrouping(n, [[t[c][1] for t in tuples] for c in range(len(cols))], [[int(t[c][0]) for t in tuples] for c in range(len(cols))],
                         [sts for _, sts in columns], first_row, [len(m) for m in members], codes, aggs)


def key_bytes(g, kinds):
    """per column: STRING: the bytes of the entries over all groups; INT, UINT: 8 * groups; BOOL: groups"""
    return [sum(len(k) for k in keys if k is not None) if kind == COL_STRING else (g.groups if kind == CW.COL_BOOL else 8 * g.groups)
            for keys, kind in zip(g.keys, kinds)]


def arrays(g, v, kind):
    return AW.record_arrays(g.aggs[v], kind)
