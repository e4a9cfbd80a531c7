"""The reference's way one level further down, restated on (Tape, Strings.B, Message) arrays -- the checker of the device unnest
sjhip_unnest_rows / sjhip_fetch_row_parents (test infrastructure, like rows_walk.py, on rows_walk.RowWalk).

  unnest_rows    per parent row: FindElement(path...) from the row's value -> Iter.Array (list_walk.array_at) -> Array.Iter and
                 Advance over the elements, one after another (parsed_array.go:27-60) -- the loop inside the loop over the outer
                 elements.  An empty path: Iter.Array on the row's own value.
                 rw: the RowWalk of the parent rows; row_offsets / record_status: the selection they belong to, as
                 rows_walk.select_rows returns them (None, None: no selection -- rw's rows are then the root values of the
                 records, record r owns row r and every status is OK).
                 -> (row_offsets [records + 1], row_index [rows], record_status [records],
                     parent_offsets [parents + 1], parent [rows], parent_status [parents])
  record_rows    the RowWalk of the root values of w's records: the parents of an unnest without a selection

Pinned by tests/test_unnest_walk.py."""
import column_walk as CW
import list_walk as LW
from query_walk import MASK
from rows_walk import RowWalk


def record_rows(w):
    return RowWalk(w, [root + 1 for root in w.records()])


def unnest_rows(rw, path, row_offsets=None, record_status=None):
    parents = rw.records()
    if row_offsets is None:
        row_offsets, record_status = list(range(len(parents) + 1)), [CW.COL_OK] * len(parents)
    index, parent, poffs, psts = [], [], [0], []
    for p, root in enumerate(parents):
        if len(path) == 0:  # Iter.Array on the row's value (parsed_json.go:1022-1025)
            tag = chr(rw.t[root + 1] >> 56)
            v, st = (root + 1, CW.COL_OK) if tag == "[" else (None, CW.COL_NULL if tag == "n" else CW.COL_TYPE)
        else:
            v, st = LW.array_at(rw, root, path)
        if v is not None:
            i, end = v + 1, (rw.t[v] & MASK) - 1
            while i < end:  # Array.Iter / Advance: a container element is one element
                index.append(i)
                parent.append(p)
                i = rw.skip(i)
        poffs.append(len(index))
        psts.append(st)
    offs = [poffs[int(o)] for o in row_offsets]  # record r owns what came from the rows it owned
    return offs, index, [int(s) for s in record_status], poffs, parent, psts
