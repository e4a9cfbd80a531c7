"""The reference's way to a row predicate, restated on (Tape, Strings.B, Message) arrays -- the checker of the device call
sjhip_where_path and of the ordering / prefix operators of sjhip_count_where_path (test infrastructure, like rows_walk.py, on
rows_walk.RowWalk / query_walk.Walk).

  satisfies   the element at a tape index against (op, want): the operators of query_walk.Walk.element_is as they are; the ordering
              operators convert the element with column_walk.convert -- Iter.Int / Uint / Float, with the amd64 results at 2^63 and
              2^64 -- and compare as Go compares two int64 / uint64 / float64, an element whose conversion is not OK satisfying
              nothing; PREFIX_STRING is bytes.HasPrefix(Iter.StringBytes, want)
  where       one call: the rows of the selection (row_offsets, row_index, statuses) -- None: no selection, record r owns one row,
              its root value, every status OK -- whose element at the path (an empty path: the row's own value) exists and
              satisfies, or with negate exactly the others; every record keeps the matching ones among the rows it owned
              -> (row_offsets, row_index, statuses)

Pinned by tests/test_where_walk.py."""
import column_walk as CW
import query_walk as Q
import rows_walk as RW

(OP_LT_INT, OP_LE_INT, OP_GT_INT, OP_GE_INT, OP_LT_UINT, OP_LE_UINT, OP_GT_UINT, OP_GE_UINT,
 OP_LT_FLOAT, OP_LE_FLOAT, OP_GT_FLOAT, OP_GE_FLOAT, OP_PREFIX_STRING) = range(7, 20)
ORDER_OPS = list(range(OP_LT_INT, OP_GE_FLOAT + 1))
ALL_OPS = list(range(0, OP_PREFIX_STRING + 1))
KIND_OF = {op: (CW.COL_INT, CW.COL_UINT, CW.COL_FLOAT)[(op - OP_LT_INT) // 4] for op in ORDER_OPS}
RELATION = ("<", "<=", ">", ">=")


def satisfies(w, v, op, want=None):
    if op <= Q.OP_IS_NULL:
        return bool(w.element_is(v, op, want))
    if op == OP_PREFIX_STRING:
        return chr(w.t[v] >> 56) == '"' and w.string_at(v).startswith(want)
    kind = KIND_OF[op]
    st, bits = CW.convert(w, v, kind)
    if st != CW.COL_OK:
        return False
    if kind == CW.COL_INT:
        got, want = (bits - (1 << 64) if bits >= 1 << 63 else bits), int(want)
    elif kind == CW.COL_UINT:
        got, want = bits, int(want)
    else:
        got, want = CW.bits2f(bits), float(want)
    rel = RELATION[(op - OP_LT_INT) % 4]
    return {"<": got < want, "<=": got <= want, ">": got > want, ">=": got >= want}[rel]


def records_selection(w):
    """what a predicate narrows when there is no selection: record r owns one row, its root value"""
    roots = w.records()
    return list(range(len(roots) + 1)), [r + 1 for r in roots], [CW.COL_OK] * len(roots)


def where(w, sel, path, op, want=None, negate=False):
    offs, index, sts = records_selection(w) if sel is None else sel
    rw = RW.RowWalk(w, index)
    before, new_index = [0], []  # before[i]: the kept rows in front of row i
    for v0 in rw.rows:
        if len(path):
            v = rw.find_path(v0 - 1, list(path))
            ok = v < Q.NOT_OBJECT and satisfies(w, v, op, want)
        else:
            ok = satisfies(w, v0, op, want)
        if bool(ok) != bool(negate):
            new_index.append(v0)
        before.append(len(new_index))
    return [before[o] for o in offs], new_index, list(sts)
