"""The reference's way to an "order by <key>, <key>, ... limit k", restated on (Tape, Strings.B, Message) arrays -- the checker of the
device call sjhip_order_paths (test infrastructure, like order_walk.py and order_strings_walk.py, on rows_walk.RowWalk).

What a caller of the reference writes is a loop over the rows -- FindElement(path...) and Iter.Float / Int / Uint / StringBytes per
key column --, a stable sort of the row numbers by the tuple, and a slice of the first k.

  columns    the key and the status of every row on every column: aggregate_walk.column for a numeric kind, group_walk.key_column
             for COL_STRING -- what the single-key checkers read
  rank       the model: successive STABLE sorts from the last column to the first, each order_walk.rank / order_strings_walk.rank on
             the column taken through the ranking so far.  The opposite route to the device's, which refines from column 0 on
  order      one call on the selection `sel` (None: no selection): the rank, the rows of rank < limit kept (0: all), the narrowing
             through where_walk.where as order_walk.order does it.  -> order_walk.Ordering with values = None and status = the
             status ON COLUMN 0 of the kept rows in rank order
  class_key, stays   csrc/sj_order.h mkord_class_key and mkord_stays
  plan       the device's plan, serially: classes of tied rows, the missing bit in the second sort's key, a numeric column's one round
             and a string column's rounds of 7 bytes, the boundary bytes, the rebuild of the active entries between columns.  -> (the
             rows in rank order, the rows every column evaluated, the rounds every column ran).  test_order_multi_walk.py holds it
             against rank

Pinned by tests/test_order_multi_walk.py and tests/test_order_multi_abi.py."""
import aggregate_walk as AW
import column_walk as CW
import group_walk as GW
import order_strings_walk as SW
import order_walk as OW
import query_walk as Q
import rows_walk as RW
import where_walk as WW

COL_STRING = SW.COL_STRING
ORDER_DESC = OW.ORDER_DESC
ORDER_MAX_KEYS = 8
U64 = OW.U64


def columns(w, index, cols):
    """cols: [(path, kind, descending)] -> [(kind, descending, keys, statuses)] over the rows whose values lie at `index`"""
    rw = RW.RowWalk(w, index)
    out = []
    for path, kind, desc in cols:
        keys, sts = GW.key_column(rw, path, COL_STRING) if kind == COL_STRING else AW.column(rw, path, kind)
        out.append((kind, bool(desc), list(keys), [int(s) for s in sts]))
    return out


def rank(data, n):
    """data: what columns returns -> the row numbers in rank order"""
    ranked = list(range(n))
    for kind, desc, keys, sts in reversed(data):
        k, s = [keys[r] for r in ranked], [sts[r] for r in ranked]
        by = SW.rank(k, s, desc) if kind == COL_STRING else OW.rank(k, s, kind, desc)
        ranked = [ranked[i] for i in by]
    return ranked


def order(w, sel, cols, limit=0):
    offs, index, sts = WW.records_selection(w) if sel is None else sel
    index = [int(i) for i in index]
    data = columns(w, index, cols)
    ranked = rank(data, len(index))
    n = len(ranked)
    kept = ranked if limit == 0 or limit >= n else ranked[:limit]
    selection = WW.where(OW._Kept(w, {index[r] for r in kept}), (offs, index, sts), (), Q.OP_EXISTS)
    number = {old: new for new, old in enumerate(sorted(kept))}  # the row numbers of the new selection
    return OW.Ordering(len(offs) - 1, selection, [number[r] for r in kept], None, [data[0][3][r] for r in kept])


def class_key(cls, missing):
    return (cls << 1 | (1 if missing else 0)) & 0xFFFFFFFF


def stays(missing, alone, chunk_full):
    return not missing and not alone and chunk_full


def plan(data, n):
    """data: what columns returns -> (rows in rank order, [the sorted rows column c evaluated], [the rounds column c ran])"""
    perm = list(range(n))
    bnd = [0] * (n + 1)
    bnd[0] = bnd[n] = 1
    active = [(r, r, 1) for r in range(n)]  # (row, position, class) in position order
    evaluated, rounds = [], []
    for c, (kind, desc, keys, sts) in enumerate(data):
        if c > 0:  # the rebuild: whoever is not alone in its class
            active, cl = [], 0
            for p in range(n):
                cl += bnd[p]
                if not (bnd[p] and bnd[p + 1]):
                    active.append((perm[p], p, cl))
            if not active:
                break
        evaluated.append(sorted(row for row, _, _ in active))
        string = kind == COL_STRING
        ok = {row: sts[row] == CW.COL_OK for row, _, _ in active}
        bound = SW.max_rounds(max([len(keys[row]) for row in ok if ok[row]] or [0])) if string else 1
        ran = 0
        while len(active) >= 2:
            def chunk(row):
                if not ok[row]:
                    return 0
                if string:
                    return SW.chunk(keys[row], SW.CHUNK * ran, desc)
                k = AW.key(keys[row], kind)
                return ~k & U64 if desc else k
            ck = [chunk(row) for row, _, _ in active]
            cls = [class_key(cl, not ok[row]) for row, _, cl in active]
            assert all(x < 1 << 32 for x in cls)
            by = sorted(range(len(active)), key=lambda i: (cls[i], ck[i]))  # stable
            head = [i == 0 or (cls[by[i]], ck[by[i]]) != (cls[by[i - 1]], ck[by[i - 1]]) for i in range(len(by))]
            nxt, cl = [], 0
            for i, e in enumerate(by):
                row, pos = active[e][0], active[i][1]
                perm[pos] = row
                if head[i]:
                    bnd[pos] = 1
                    cl += 1
                alone = head[i] and (i + 1 == len(by) or head[i + 1])
                full = string and ((~ck[e] if desc else ck[e]) & 0xFF) == SW.CHUNK
                if stays(not ok[row], alone, full):
                    nxt.append((row, pos, cl))
            active = nxt
            ran += 1
            if ran >= bound:
                assert not active, "entries are left behind the bound of the longest key"
                break
        rounds.append(ran)
    return perm, evaluated, rounds
