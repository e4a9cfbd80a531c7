"""The documents of the member-row tests (tests/test_members_walk.py pins the serial model and the parity claim on every one of
them; tests/test_gpu_members.py and tests/test_debug_bounds_members.py run the device on them).  Each entry of DOCS is
(name, document, ndjson, [step, ...]): a step is ("select", path), ("members", path) or ("unnest", path), applied in order to the
selection in force (none at first)."""
TILE = 2048  # TW_TILE of csrc/sj_tapewalk.h
SEAM_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)  # tests/test_gpu_rows.py
# integers whose raw word's top byte is a tag (tests/test_gpu_rows.py RAW)
RAW = {"[": 6557241057451442176, "{": 8863084066665136128, "]": 6701356245527298048, "}": 9007199254740992000,
       "l": 7782220156096217088, '"': 2449958197289549824}

OK, NOT_FOUND, NOT_OBJECT, TYPE, NULL, RANGE = range(6)

# one NDJSON input whose parent rows -- the elements of "o" -- hit every status under the path ("a",); duplicate names, "" as a
# name, escaped names, an array of an odd number of strings and scalars as targets, {} between non-empty objects
STATUS_DOC = b"\n".join([
    b'{"o":[{"a":{"x":1,"y":{"x":2},"x":[3,{"q":4}]}},{"z":1},{"a":null},{"a":"s"},5,[{"a":{"k":1}}],{"a":{}},{"a":[1,"a","b"]},'
    b'{"b":2,"a":{"":true,"a\\"b":"a\\"b","\\u00e9\\n":null}}]}',
    b'{"o":null}',
    b'{"o":[]}',
    b'{"o":[{"a":{"d":"d","d":"x"},"a":{"n":0}},{"a":[1],"a":{"m":4}}]}',  # duplicate keys on the way: the first wins
])
STATUS_PARENTS = [OK, NOT_FOUND, NULL, TYPE, NOT_OBJECT, NOT_OBJECT, OK, TYPE, OK, OK, TYPE]
STATUS_WANT = ([0, 6, 6, 6, 8], [OK, NULL, OK, OK],                        # the records: new row offsets, statuses kept
               [0, 3, 3, 3, 3, 3, 3, 3, 3, 6, 8, 8], STATUS_PARENTS,        # the parents: offsets over the new rows, statuses
               [0, 0, 0, 8, 8, 8, 9, 9], 'l{[t"n""',                        # the new rows: their parent, their tag
               [b"x", b"y", b"x", b"", b'a"b', "é\n".encode(), b"d", b"d"])  # ... and their names

KINDS_DOC = b'[{"a":1,"b":{"c":2}},{},[1,2],"s",null,7,{"k":{"k":{"z":[]}}},["x","y","z"],{"":{}}]'  # parents of every kind, no keys
MAP_OF_MAPS = b'{"m":{"a":{"x":1,"y":2},"b":{},"c":{"z":{"w":3}},"d":[{"q":1}],"e":"e","a":{"y":5}}}'
ARRAY_OF_OBJECTS = b'{"items":[{"id":1,"name":"n1","t":[1,2]},{},{"id":2},7,{"id":3,"id":4,"o":{"id":5}}]}'


def member_value(j):
    """values of every shape: a literal, a number, a string equal to its own name, nested containers (whose members and elements
    must not be counted), an array of an odd number of strings, an integer whose raw word looks like a tag"""
    v = j % 7
    if v == 0:
        return "true"
    if v == 1:
        return str(j * 37 - 5)
    if v == 2:
        return '"m%d"' % j
    if v == 3:
        return '{"m1":%d,"x":{"y":[%d,{"m2":0}]}}' % (j, j)
    if v == 4:
        return '["m1","m2","m3"]'
    if v == 5:
        return str(list(RAW.values())[j % 6])
    return "{}"


def members_text(n, first=0):
    return ",".join('"m%d":%s' % (j, member_value(j)) for j in range(first, first + n))


def seam_doc(key_at, varied=60, flat=3000):
    """one document whose object "m" has the tag word of its first member's key at tape word key_at:
    r { "p" [ pad ] "m" { "m0" ...; behind `varied` members of every shape, `flat` members of three words each (key, length, a
    literal) span more than four tiles, and two of every three tile cuts fall between a key's tag word and its value (2048 is no
    multiple of 3): those tiles hold an odd number of starts"""
    extra = key_at - 9
    assert extra >= 0
    pad = ["0"] * (extra // 2) + ["true"] * (extra % 2)
    tail = ",".join('"f%d":%s' % (j, ("true", "null", "false")[j % 3]) for j in range(flat))
    return ('{"p":[%s],"m":{%s,%s},"q":{"m0":1}}' % (",".join(pad), members_text(varied), tail)).encode()


SEAM_KEYS = [TILE - 14, TILE - 4, TILE - 3, TILE - 2, TILE - 1, TILE, TILE + 1]


def one_object_doc(n):
    return ('{"n":%d,"m":{%s}}' % (n, members_text(n))).encode()


def spread_doc(n):
    """n members spread over objects of 0 to 7 members, the elements of "items" """
    items, at, k = [], 0, 0
    while at < n:
        take = min((k * 5 + 3) % 8, n - at)
        items.append("{%s}" % members_text(take, at))
        at += take
        k += 1
    return ('{"items":[%s]}' % ",".join(items)).encode()


def nested_lines(n_records):
    """record r owns (r * 5) % 8 parents -- the elements of "items" --; parent j of it holds in "o" an object of (j * 3 + r * 2) % 8
    members, or -- every fifth -- null, a number, an array of three strings, or nothing at all"""
    lines = []
    for r in range(n_records):
        items = []
        for j in range((r * 5) % 8):
            k = r * 8 + j
            if k % 5 == 4:
                o = ("null", "7", '["a","b","c"]', None)[(k // 5) % 4]
            else:
                o = "{%s}" % members_text((j * 3 + r * 2) % 8, k)
            items.append('{"id":%d%s,"u":{"m1":[9]}}' % (k, "" if o is None else ',"o":' + o))
        lines.append('{"k":%d,"items":[%s]}' % (r, ",".join(items)))
    return "\n".join(lines).encode()


def anchor_doc():
    """a pad of 1100 integers whose tag AND raw word look like two-word tags (l): the tile that starts at word 2048 finds no anchor
    among the 64 words in front of it and the global anchors decide, under the member passes; the members' values are integers
    whose raw word looks like { } [ ] l and the string tag"""
    lit = str(RAW["l"])
    vals = list(RAW.values())
    members = ",".join('"r%d":%d' % (j, vals[j % 6]) for j in range(900))
    return ('{"p":[%s],"m":{%s,"o":{"r1":%s},"a":[%s,%s,%s]}}' % (",".join([lit] * 1100), members, lit, lit, lit, lit)).encode()


NAME_LENGTHS = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 512)


def names_doc():
    """names of every length around the lane / wave copy switch (32) and the 64-byte step, escaped names, duplicates"""
    names = ["n" * ln for ln in NAME_LENGTHS] + ['a\\"b', "\\u00e9\\n", "t\\tab" + "x" * 40, "dup", "dup", "n" * 33, "\\\\", "git-a", "git", "gi"]
    return ('{"m":{%s}}' % ",".join('"%s":%d' % (nm, k) for k, nm in enumerate(names))).encode()


def parking_lines(n=400):
    import fixtures
    return b"\n".join(fixtures.load("parking-citations").split(b"\n")[:n])


def sharded_lines(n=9000):
    """NDJSON lines of a map of 0 to 7 members each and, behind it, an array of three strings at the members' depth -- an odd number
    of tag words that are no starts: parity is a matter of the targets alone, and restarts with every part"""
    lines = []
    for k in range(n):
        lines.append('{"id":%d,"m":{%s},"pad":"%s","s":["a","b","c"]}' % (k, members_text((k * 3) % 8, k), "x" * 150))
    return "\n".join(lines).encode()


DOCS = [
    ("status", STATUS_DOC, True, [("select", (b"o",)), ("members", (b"a",))]),
    ("status records", STATUS_DOC, True, [("members", (b"o",))]),
    ("kinds", KINDS_DOC, False, [("select", ()), ("members", ())]),
    ("kinds keyed", KINDS_DOC, False, [("select", ()), ("members", (b"k",)), ("members", ())]),
    ("map of maps", MAP_OF_MAPS, False, [("members", (b"m",)), ("members", ())]),
    ("array of objects", ARRAY_OF_OBJECTS, False, [("select", (b"items",)), ("members", ())]),
    ("root object", MAP_OF_MAPS, False, [("members", ())]),
    ("names", names_doc(), False, [("members", (b"m",))]),
    ("anchor", anchor_doc(), False, [("members", (b"m",))]),
    ("0 to 7", nested_lines(300), True, [("select", (b"items",)), ("members", (b"o",))]),
] + [("seam %d" % k, seam_doc(k), False, [("members", (b"m",))]) for k in SEAM_KEYS] \
  + [("one object %d" % n, one_object_doc(n), False, [("members", (b"m",))]) for n in SEAM_COUNTS] \
  + [("spread %d" % n, spread_doc(n), False, [("select", (b"items",)), ("members", ())]) for n in SEAM_COUNTS]
