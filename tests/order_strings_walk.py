"""The reference's way to an "order by <string> limit k", restated on (Tape, Strings.B, Message) arrays -- the checker of the device
call sjhip_order_path_strings (test infrastructure, like order_walk.py, on rows_walk.RowWalk / query_walk.Walk).

What a caller of the reference writes is a loop over the rows -- FindElement(path...) and Iter.StringBytes --, a stable sort of the
row numbers with bytes.Compare, and a slice of the first k.

  rank       the row numbers in rank order: Python's stable sorted() on (not ok, key bytes) -- bytes compare as bytes.Compare does:
             unsigned, from the left, a proper prefix first.  Descending: a stable sort by the DESCENDING RANK OF THE DISTINCT KEYS,
             not the list reversed: equal keys stay in row order in both directions, the rows without an OK key are last in both
  order      one call on the selection `sel` (None: no selection): key and status of every row from group_walk.key_column (the
             string key of the grouping: CW.text without conversion), the rank, the rows of rank < limit kept (0: all), the
             narrowing through where_walk.where as order_walk.order does it.  -> order_walk.Ordering with values = the key bytes of
             the kept rows in rank order (None where not OK): what extract_path_strings taken through `order` must give
  chunk      csrc/sj_order.h strord_chunk: the 7 key bytes at `at` big-endian, zero padded, above the count of the key's own bytes
  refine     the device's plan, serially: rounds of 7 bytes, each a stable sort of the active entries by (class, chunk key), new
             classes where the chunk key changes, an entry active while its class has company and its chunk was full.  -> (the OK
             rows in rank order, the rounds that sorted).  test_order_strings_walk.py holds it against rank

Pinned by tests/test_order_strings_walk.py and tests/test_order_strings_abi.py."""
import column_walk as CW
import group_walk as GW
import order_walk as OW
import query_walk as Q
import where_walk as WW

COL_STRING = GW.COL_STRING
ORDER_DESC = OW.ORDER_DESC
CHUNK = 7
U64 = (1 << 64) - 1


def rank(keys, sts, descending=False):
    """keys: bytes (anything where the status is not OK)"""
    ok = [st == CW.COL_OK for st in sts]
    if not descending:
        return sorted(range(len(keys)), key=lambda r: (not ok[r], bytes(keys[r]) if ok[r] else b""))
    distinct = sorted({bytes(keys[r]) for r in range(len(keys)) if ok[r]}, reverse=True)
    number = {k: i for i, k in enumerate(distinct)}
    return sorted(range(len(keys)), key=lambda r: (not ok[r], number[bytes(keys[r])] if ok[r] else 0))


def order(w, sel, path, descending=False, limit=0):
    import rows_walk as RW
    offs, index, sts = WW.records_selection(w) if sel is None else sel
    index = [int(i) for i in index]
    keys, ksts = GW.key_column(RW.RowWalk(w, index), path, COL_STRING)
    ranked = rank(keys, ksts, descending)
    n = len(ranked)
    kept = ranked if limit == 0 or limit >= n else ranked[:limit]
    selection = WW.where(OW._Kept(w, {index[r] for r in kept}), (offs, index, sts), (), Q.OP_EXISTS)
    number = {old: new for new, old in enumerate(sorted(kept))}  # the row numbers of the new selection
    return OW.Ordering(len(offs) - 1, selection, [number[r] for r in kept], [keys[r] for r in kept], [ksts[r] for r in kept])


def chunk(key, at, descending=False):
    part = bytes(key[at:at + CHUNK])
    k = int.from_bytes(part + bytes(CHUNK - len(part)), "big") << 8 | len(part)
    return ~k & U64 if descending else k


def max_rounds(longest):
    return longest // CHUNK + 1


def refine(keys, descending=False):
    """keys: the bytes of the OK rows in row order -> (their row numbers in rank order, the rounds that ran)"""
    perm = list(range(len(keys)))
    active = [(r, r, 0) for r in perm]  # (row, position, class) in position order
    rounds = 0
    while len(active) > 1:
        assert rounds < max_rounds(max(map(len, keys)))
        ck = [chunk(keys[row], CHUNK * rounds, descending) for row, _, _ in active]
        by = sorted(range(len(active)), key=lambda i: (active[i][2], ck[i]))  # stable
        head = [i == 0 or (active[by[i]][2], ck[by[i]]) != (active[by[i - 1]][2], ck[by[i - 1]]) for i in range(len(by))]
        nxt, cls = [], 0
        for i, e in enumerate(by):
            row, pos = active[e][0], active[i][1]
            perm[pos] = row
            cls += head[i]
            alone = head[i] and (i + 1 == len(by) or head[i + 1])
            count = (~ck[e] if descending else ck[e]) & 0xFF
            if not alone and count == CHUNK:
                nxt.append((row, pos, cls))
        active = nxt
        rounds += 1
    return perm, rounds
