"""The reference's way into an object, restated on (Tape, Strings.B, Message) arrays -- the checker of the device member rows
sjhip_unnest_members / sjhip_extract_row_names / sjhip_where_row_names (test infrastructure, like unnest_walk.py, on
rows_walk.RowWalk).

  object_at        FindElement(path...) from the row's value -> Iter.Object (parsed_json.go: "next item is not object")
  unnest_members   per parent row: object_at, then the Object.NextElementBytes loop (parsed_object.go) -- name, value, skip the
                   value, one member after another; duplicate names are visited each.  An empty path: Iter.Object on the row's own
                   value.  rw, row_offsets, record_status: as unnest_walk.unnest_rows takes them.
                   -> unnest_rows' six arrays (the rows are the members' VALUES) + names [rows]: the unescaped name of every row
  names_of         the name of every row of a member selection, read back from the tape alone: the string two words in front of
                   the row's value (what a narrowing keeps)
  member_starts    the claim the device's tile pass rests on, enumerated: every tag word at the rows' depth strictly inside the
                   target of an OK parent, in tape order -- keys and values, alternating

Pinned by tests/test_members_walk.py."""
import column_walk as CW
from query_walk import MASK, NOT_OBJECT


def object_at(rw, root, path):
    """-> (index of the object's '{' word, COL_OK) or (None, status)"""
    v = rw.find_path(root, list(path)) if len(path) else root + 1
    if v == NOT_OBJECT:
        return None, CW.COL_NOT_OBJECT
    if v > NOT_OBJECT:
        return None, CW.COL_NOT_FOUND
    tag = chr(rw.t[v] >> 56)
    if tag == "n":
        return None, CW.COL_NULL
    if tag != "{":
        return None, CW.COL_TYPE
    return v, CW.COL_OK


def unnest_members(rw, path, row_offsets=None, record_status=None):
    parents = rw.records()
    if row_offsets is None:
        row_offsets, record_status = list(range(len(parents) + 1)), [CW.COL_OK] * len(parents)
    index, parent, names, poffs, psts = [], [], [], [0], []
    for p, root in enumerate(parents):
        v, st = object_at(rw, root, path)
        if v is not None:
            i, end = v + 1, (rw.t[v] & MASK) - 1
            while i < end:  # NextElementBytes: the name, then the value; a container value is one member
                assert chr(rw.t[i] >> 56) == '"'
                names.append(rw.string_at(i))
                index.append(i + 2)
                parent.append(p)
                i = rw.skip(i + 2)
        poffs.append(len(index))
        psts.append(st)
    offs = [poffs[int(o)] for o in row_offsets]  # record r owns what came from the rows it owned
    return offs, index, [int(s) for s in record_status], poffs, parent, psts, names


def names_of(w, index):
    return [w.string_at(int(i) - 2) for i in index]


def _tag_words(t):
    """the tag words of the tape, in order (a number's and a string's second word is no tag word) with their depth below the root"""
    i, depth = 0, 0
    while i < len(t):
        tag = chr(t[i] >> 56)
        if tag in "}]":
            depth -= 1
        if tag != "r":
            yield i, tag, depth  # (a root value lies at 0)
        if tag in "{[":
            depth += 1
        i += 2 if tag in '"lud' else 1


def member_starts(rw, path, depth):
    """depth: of the NEW rows below their record's root value -> [(tape index, tag)] of the starts"""
    ranges = []
    for root in rw.records():
        v, st = object_at(rw, root, path)
        if v is not None:
            ranges.append((v, (rw.t[v] & MASK) - 1))
    out, k = [], 0
    for i, tag, d in _tag_words(rw.t):
        while k < len(ranges) and ranges[k][1] <= i:
            k += 1
        if k < len(ranges) and ranges[k][0] < i and d == depth and tag not in "}]":
            out.append((i, tag))
    return out
