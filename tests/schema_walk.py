"""The reference's way to the schema of a row set, restated on (Tape, Strings.B, Message) arrays -- the checker of the device row
schema sjhip_row_schema / sjhip_fetch_row_schema (test infrastructure, like members_walk.py, on rows_walk.RowWalk).

  row_schema   per row: members_walk.object_at (FindElement(path...) -> Iter.Object), then the Object.NextElementBytes loop -- name,
               value, skip the value --; a name not seen before is appended to the dictionary, and the member is counted under
               (its name, the Type of its value's tag as TagToType maps it).  A duplicate name inside one object counts each time.
               An empty path: Iter.Object on the row's own value.
               -> (rows, status [6]: the rows per COL_* status, members, names: the unescaped names in first-occurrence order,
                  first_row [names]: the first row that has the name, counts [names][8]: column T - 1 counts the values of type T)
  type_of_tag  TagToType (parsed_json.go) on the tag byte of a value

Pinned by tests/test_schema_walk.py."""
import column_walk as CW
from members_walk import object_at
from query_walk import MASK

TYPE_NULL, TYPE_STRING, TYPE_INT, TYPE_UINT, TYPE_FLOAT, TYPE_BOOL, TYPE_OBJECT, TYPE_ARRAY = range(1, 9)
SCHEMA_TYPES = 8
_TAG_TYPES = {"n": TYPE_NULL, '"': TYPE_STRING, "l": TYPE_INT, "u": TYPE_UINT, "d": TYPE_FLOAT, "t": TYPE_BOOL, "f": TYPE_BOOL,
              "{": TYPE_OBJECT, "[": TYPE_ARRAY}


def type_of_tag(tag):
    return _TAG_TYPES[tag]


def row_schema(rw, path):
    status = [0] * (CW.COL_RANGE + 1)
    code, names, first_row, counts, members = {}, [], [], [], 0
    parents = rw.records()
    for p, root in enumerate(parents):
        v, st = object_at(rw, root, path)
        status[st] += 1
        if v is None:
            continue
        i, end = v + 1, (rw.t[v] & MASK) - 1
        while i < end:  # NextElementBytes: the name, then the value; a container value is one member
            assert chr(rw.t[i] >> 56) == '"'
            name = rw.string_at(i)
            k = code.get(name)
            if k is None:
                k = code[name] = len(names)
                names.append(name)
                first_row.append(p)
                counts.append([0] * SCHEMA_TYPES)
            counts[k][type_of_tag(chr(rw.t[i + 2] >> 56)) - 1] += 1
            members += 1
            i = rw.skip(i + 2)
    return len(parents), status, members, names, first_row, counts
