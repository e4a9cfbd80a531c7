"""The reference's way to the rows of a document, restated on (Tape, Strings.B, Message) arrays -- the checker of the device row
selection sjhip_select_rows / sjhip_fetch_rows (test infrastructure, like list_walk.py, on query_walk.Walk).

  select_rows    per record: FindElement(path...) (query_walk.Walk.find_path) -> Iter.Array (list_walk.array_at) -> Array.Iter and
                 Advance over the elements, one after another (parsed_array.go:27-60) -- the serial walk the device replaces by
                 passes over the tape.  An empty path: Iter.Array on the record's root value.
                 -> (row_offsets [records + 1], row_index [rows]: the tape index of every row's value, statuses [records])
  RowWalk        a Walk whose records() are the rows: column_walk, list_walk and table_walk start at records()[r] + 1, the value
                 of the record's root, so on a RowWalk they run from the value of every row instead -- unchanged

Pinned by tests/test_rows_walk.py."""
import column_walk as CW
import list_walk as LW
import table_walk as TW
from query_walk import MASK, Walk


def select_rows(w, path):
    offs, index, sts = [0], [], []
    for root in w.records():
        if len(path) == 0:  # Iter.Array on the root value (parsed_json.go:1022-1025)
            tag = chr(w.t[root + 1] >> 56)
            v, st = (root + 1, CW.COL_OK) if tag == "[" else (None, CW.COL_NULL if tag == "n" else CW.COL_TYPE)
        else:
            v, st = LW.array_at(w, root, path)
        if v is not None:
            i, end = v + 1, (w.t[v] & MASK) - 1
            while i < end:  # Array.Iter / Advance: a container element is one element
                index.append(i)
                i = w.skip(i)
        offs.append(len(index))
        sts.append(st)
    return offs, index, sts


class RowWalk(Walk):
    """the rows of `w` (row_index: select_rows' or the device's) in the place of its records"""

    def __init__(self, w, row_index):
        self.t, self.s, self.m = w.t, w.s, w.m
        self.rows = [int(i) for i in row_index]

    def records(self):
        return [i - 1 for i in self.rows]  # (the walkers look at records()[r] + 1: the row's value)


def on_rows(w, path):
    return RowWalk(w, select_rows(w, path)[1])


# the walkers from a row's value instead of a record's root (rw: a RowWalk)
def find_path(rw, path):
    return [rw.find_path(r, list(path)) for r in rw.records()]


def count_where_path(rw, path, op, want=None):
    hits = 0
    for r in rw.records():
        v = rw.find_path(r, list(path))
        hits += v < CW.NOT_OBJECT and bool(rw.element_is(v, op, want))
    return hits


def project_keys(rw, keys):
    return [rw.project_keys(r, list(keys)) for r in rw.records()]


def column(rw, path, kind):
    return CW.column(rw, path, kind)


def string_column(rw, path, cvt):
    return CW.string_column(rw, path, cvt)


def list_column(rw, path, kind):
    return LW.list_column(rw, path, kind)


def list_string_column(rw, path, cvt):
    return LW.list_string_column(rw, path, cvt)


def table(rw, columns):
    return TW.table(rw, columns)
