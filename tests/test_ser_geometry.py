"""CPU: the documents of tests/ser_geometry.py lie where they claim to lie and the model says what the oracle says.

For every document the oracle parses it, the model's tape is the oracle's word for word, the model's plain stream is the
oracle's Serialize without de-duplication byte for byte, and the model's de-duplicating stream is read by the oracle's
Deserialize to a tape that marshals to the same text and passes the hash-free checker -- so the references of
tests/test_gpu_serialize_seams.py agree before the device is asked.  The coverage tests compute, from the documents' words, which
cut of k_ser_tile / k_des_tile each reaches and name every case that is missing; the constants the placements rest on are pinned
to the literals in csrc/serialize.hip and csrc/sj_tapewalk.h; the oracle's verdict on every corrupt stream is recorded here."""
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
import ser_geometry as S

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simdjson-go_amd", "csrc")


@functools.lru_cache(maxsize=None)
def ref(f, i):
    """the oracle's parse of document i of a family and its plain stream -> (Parsed, message, stream)"""
    d = S.family(f)[i]
    r = O.parse(d.data, ndjson=d.nd, copy_strings=True)
    assert r.rc == 0, d.name
    msg = bytes(d.data[r.msg_off:r.msg_off + r.msg_len])
    return r, msg, O.serialize(r.tape, r.strings, msg, dedup=False)[0].tobytes()


@pytest.mark.parametrize("f", sorted(S.FAMILIES))
def test_model_against_the_oracle(f):
    assert S.family(f)
    for i, d in enumerate(S.family(f)):
        r, msg, want = ref(f, i)
        if d.big:
            assert len(r.strings) == 0 and len(r.tape) == d.info.get("n", len(r.tape)), d.name
            continue
        assert len(r.tape) == d.n and np.array_equal(d.tape, r.tape), d.name
        assert r.strings.tobytes() == d.strings_b, d.name
        assert d.stream(False) == want, S.describe(d, want, False)
        dd = d.stream(True)
        rc, tape2, strs2, msg2 = O.deserialize(dd)
        assert rc == 0, d.name
        rc, a = O.marshal_json(tape2, strs2, bytes(msg2))
        rc2, b = O.marshal_json(r.tape, r.strings, msg)
        assert rc == 0 and rc2 == 0 and a == b, d.name
        assert S.valid_dedup(dd, d) == [], (d.name, S.valid_dedup(dd, d)[:3])
        assert S.valid_dedup(d.stream(False), d) == [], d.name  # (keeping everything is a policy too)
        assert len(dd) <= len(want)
        k = len(want) // 2  # the reporter names the owner of a byte
        assert S.describe(d, want[:k] + bytes([want[k] ^ 1]) + want[k + 1:], False)[6] == k


def test_the_checker_rejects_wrong_columns():
    d = next(x for x in S.family("c") if x.info.get("order") == "ABBAB")
    kept, target = d.plan
    strs = [k for k, _ in d.strs]  # A B B A B
    assert kept == {strs[0], strs[1], strs[2], strs[4]} and target == {strs[3]: strs[0]}
    assert S.valid_dedup(d.stream_with((set(strs), {})), d) == []
    assert S.valid_dedup(d.stream_with(({strs[0], strs[1]}, {strs[2]: strs[1], strs[3]: strs[0], strs[4]: strs[1]})), d) == []
    # a dropped first occurrence: the column holds the second copy of a string, behind other strings, and the first points at it
    e = S.family("b")[0]
    ks = [k for k, x in e.strs if x == S.B_REPEATED[0]]
    kept, target = set(e.plan[0]), dict(e.plan[1])
    kept = kept - {ks[0]} | {ks[1]}
    target = {k: (ks[1] if t == ks[0] else t) for k, t in target.items() if k != ks[1]}
    target[ks[0]] = ks[1]
    assert S.valid_dedup(e.stream(True), e) == [] and "first occurrence" in str(S.valid_dedup(e.stream_with((kept, target)), e))
    # a repeat pointing at a later copy: the last B points at the second B, both B's in front of it kept
    assert S.valid_dedup(d.stream_with(({strs[0], strs[1], strs[2]}, {strs[3]: strs[0], strs[4]: strs[2]})), d)
    # an offset shifted by one
    u = S.unframe(d.stream(True))
    vals = np.frombuffer(u["values"], dtype=np.uint64).copy()
    scol, tags, _ = d.columns(True)
    vals[d.vstart[strs[3]] // 8] += 1
    assert S.valid_dedup(S.frame(d.n, scol, tags, vals.tobytes()), d)


def test_constants_are_the_kernels():
    ser = open(os.path.join(CSRC, "serialize.hip")).read()
    tw = open(os.path.join(CSRC, "sj_tapewalk.h")).read()
    assert "static constexpr int TW_THREADS = %d, TW_ITEMS = %d, TW_TILE = TW_THREADS * TW_ITEMS;" % (S.THREADS, S.ITEMS) in tw
    assert S.TILE == S.THREADS * S.ITEMS and S.WAVE_WORDS * 4 == S.TILE
    assert "static constexpr int ST_THREADS = TW_THREADS, ST_ITEMS = TW_ITEMS, ST_TILE = TW_TILE;" in ser
    assert "for (int k = 0; k <= ST_ITEMS; k++) w[k] = base + k < p.n ? p.tape[base + k] : 0;" in ser  # the look-ahead word
    assert "if (tid < %d) {" % S.REACH in tw and "(tb > %d ? -2ll : -1ll)" % S.REACH in tw
    assert "static constexpr int DS_THREADS = %d, DS_ITEMS = %d, DS_TILE = DS_THREADS * DS_ITEMS;" % (S.DS_THREADS, S.DS_ITEMS) in ser
    assert "static constexpr u32 SER_SLOT_BITS = %d, SER_SLOTS = 1u << SER_SLOT_BITS;" % S.SER_SLOT_BITS in ser
    assert "u64 h = 0x%xull ^ len;" % S.HASH_SEED in ser
    assert "* 0x%xull + (h >> %d);" % (S.HASH_MUL, S.HASH_SHIFT) in ser
    assert "h = (h ^ t) * 0x%xull;" % S.HASH_FIN in ser
    assert "return (u32)((h ^ (h >> %d)) >> (64 - SER_SLOT_BITS));" % S.HASH_FIN_SHIFT in ser
    assert "block_excl_sum(((unsigned long long)nv << 24) | nw, s_s, tid, &tot);" in ser
    assert "const unsigned long long packed = ((unsigned long long)nval << 20) | ntag;" in ser
    assert "const u32 per = ((n + %du) / %du + %du) / %du * %du;" % (S.SCAN_WAVES - 1, S.SCAN_WAVES, S.SCAN_ROUND - 1, S.SCAN_ROUND, S.SCAN_ROUND) in tw
    assert [S.scan_per(n) for n in (1, 16, 17, 1024, 1025)] == [64, 64, 64, 64, 128]
    assert S.ser_hash(b"") == ((S.HASH_SEED * S.HASH_FIN & S.U64) ^ ((S.HASH_SEED * S.HASH_FIN & S.U64) >> 31)) >> 44


def missing(want, got):
    return sorted(map(str, set(want) - set(got)))


def test_a_every_kind_on_every_edge():
    docs = S.family("a")
    want = {(k, e) for k in S.KINDS for e in S.A_EDGES} | {("end", e) for e in ("t2047", "t2048", "t2049")}
    assert missing(want, S.a_observed(docs)) == []
    assert missing(S.A_LENGTHS, {d.n for d in docs}) == []
    assert {1, 7, 0} <= {d.n % S.ITEMS for d in docs}  # the last thread holds 1, 7 and 8 words
    # a two-word entry on item 7 has its second word in the look-ahead slot of its thread
    d = docs[0]
    assert all(int(w) % S.ITEMS == S.ITEMS - 1 for k, w in enumerate(d.words) if d.label(k) == "e")


def test_b_anchor_distances():
    seen = set()
    for d in S.family("b"):
        obs = S.b_observed(d)
        assert d.tiles == S.B_TILES and (d.info["dist"], d.info["dist"] % 2 == 0, d.info["pos"]) in obs, d.name
        assert d.info["retry"] == (max(o[0] for o in obs) > S.REACH)
        seen |= obs
        # repeated strings in front of the tile that cannot classify, inside it and behind it
        t = d.info["edge"] // S.TILE
        for s in S.B_REPEATED:
            at = {int(d.words[k]) // S.TILE for k, x in d.strs if x == s}
            assert min(at) < t and t in at and (max(at) > t or t == S.B_TILES - 1), (d.name, s)
        kinds = {d.kinds[k] for k, w in enumerate(d.words) if d.info["edge"] - d.info["dist"] < w < d.info["edge"]}
        assert kinds == {"int", "float"}, d.name
    assert missing({(x, x % 2 == 0, p) for x in S.B_DISTANCES for p in S.B_POSITIONS}, seen) == []
    anchors = {d.kinds[list(d.words).index(d.info["edge"] - d.info["dist"])] if d.info["edge"] - d.info["dist"] in d.words else "raw"
               for d in S.family("b")}
    assert anchors == {"null", "raw"}  # (raw: the value word of a uint)


def test_c_dedup_seams():
    docs = {d.name: d for d in S.family("c")}
    d = docs["c placements"]
    first, seen, forms = {}, set(), set()
    for k, s in d.strs:
        if s in first:
            seen.add(S.placement(int(d.words[first[s]]), int(d.words[k])))
            forms.add((d.kinds[first[s]], d.kinds[k]))
            assert k in d.plan[1]
        else:
            first[s] = k
    assert missing(list(S.C_PLACEMENTS) , seen) == [] and forms >= {("str", "key"), ("key", "str"), ("str", "str")}
    assert d.data.count(b"\\u00") == 2 and sum(s == b"Ab" for _, s in d.strs) == 3
    orders = set()
    for d in S.family("c"):
        if "order" in d.info:
            a, b = d.info["A"], d.info["B"]
            assert a != b and S.ser_hash(a) == S.ser_hash(b) and (len(a) == len(b)) == (d.info["lengths"] == "equal")
            keeps = {"A": sum(s == a for k, s in d.strs if k in d.plan[0]), "B": sum(s == b for k, s in d.strs if k in d.plan[0])}
            assert keeps == d.info["keeps"], d.name
            orders.add((d.info["order"], d.info["lengths"]))
    assert orders == {(o, l) for o in ("ABBAB", "BAAB") for l in ("equal", "unequal")}
    d = docs["c lengths and near-equal pairs"]
    assert missing(S.C_LENGTHS, {len(s) for k, s in d.strs if k in d.plan[1] or not s}) == []
    keys = set()
    for key, x, y in d.info["lay"]:
        assert x != y and S.ser_hash(x) == S.ser_hash(y)
        diff = [i for i in range(min(len(x), len(y))) if x[i] != y[i]]
        if key == "prefix":
            assert not diff and len(x) != len(y)
        elif key[0] == "differ":
            assert diff == [key[2]] and len(x) == len(y) == key[1]
        else:
            assert len(x) == len(y) == key[1] and diff and diff[0] >= key[1] - 8
        kept = [s for k, s in d.strs if k in d.plan[0] and s in (x, y)]
        assert kept == [x, y, y], key  # X Y X Y: Y meets X's bytes in its slot every time
        keys.add(key)
    assert missing([("differ", n, p) for n, p in S.C_DIFFER] + [("tail", n) for n in S.C_TAILS] + ["prefix"], keys) == []
    d = docs["c alignments"]
    obs = S.c_align_observed(d)
    assert missing({(a, r) for a in range(8) for r in range(8)}, {o[:2] for o in obs}) == []
    assert missing([n for n in S.C_LENGTHS if n], {o[2] for o in obs}) == [] and set(d.info["lay"]) <= obs
    kb = S.kept_bytes_per_tile(docs["c heavy tile"])
    assert kb[1] > 65536 and kb[2] == 0 and kb[3] > 0
    assert not docs["c no string"].strs and docs["c no string"].stream(True) == docs["c no string"].stream(False)
    d = docs["c empty strings only"]
    assert len(d.strs) == 3 and S.unframe(d.stream(True))["strings"] == b""
    d = docs["c one string 3000 times"]
    assert len(d.strs) == 3000 and len(d.plan[0]) == 1 and d.tiles > 2


def test_d_packed_count_extremes():
    want = {"atoms": {"null": 1024, "true": 1024}, "openers": {"[": 1024, "]": 1024}, "strings": {"str": 1024}, "e floats": {"e": 1024}}
    for d in S.family("d"):
        assert S.d_observed(d) == want[d.info["form"]], d.name
    assert missing(S.D_FORMS, {d.info["form"] for d in S.family("d")}) == []


def test_e_every_varint_step_of_every_length():
    obs = set()
    for d in S.family("e"):
        obs |= S.e_observed(d)
    want = {(q, n) for q in ("tape", "strings", "strings dedup", "tags", "rest") for n in S.E_STEPS} | {("values", n) for n in S.E_VALUE_STEPS}
    assert missing(want, obs) == []
    assert [S.uvarint_len(n) for n in (127, 128, 16383, 16384)] == [1, 2, 2, 3]


def test_f_g_tile_counts_and_tag_edges():
    tiles = set()
    for i, d in enumerate(S.family("f")):
        tiles.add((len(ref("f", i)[0].tape) + S.TILE - 1) // S.TILE)
    assert missing(S.F_TILES, tiles) == []
    assert {S.scan_per(t) for t in S.F_TILES} == {64, 128}
    tag_tiles, counts, edges, spans = set(), set(), set(), set()
    for i, d in enumerate(S.family("g")):
        u = S.unframe(ref("g", i)[2])
        tag_tiles.add((len(u["tags"]) + S.DS_TILE - 1) // S.DS_TILE)
        counts.add(len(u["tags"]))
        if not d.big:
            assert len(u["tags"]) == len(d.kinds)
            edges |= {(d.label(k) if d.label(k) != "end" else "R", e) for k in range(len(d.kinds)) for e in S.tag_edge_classes(k)}
            spans |= S.bracket_spans(d)
    assert missing(S.G_TILES, tag_tiles) == [] and missing(S.G_TAGS, counts) == []
    assert missing({(k, e) for k in S.KINDS for e in S.G_EDGES}, edges) == []
    assert {("]", 0, 1), ("]", 0, 3), ("}", 0, 3), ("R", 0, 3), ("R", 3, 3), ("R", 4, 5)} <= spans


# the corrupt streams the oracle's Deserialize reads all the same (tests/test_gpu_serialize_seams.py: the device's verdicts)
H_ORACLE_READS = {"TagNop on the last tag of a thread", "TagNop on the last tag of a tile"}


def test_h_the_oracles_verdicts():
    d, good, muts = S.h_streams()
    assert O.deserialize(good)[0] == 0 and len({n for n, _ in muts}) == len(muts)
    reads = {name for name, s in muts if O.deserialize(s)[0] == 0}
    assert reads == H_ORACLE_READS
    for name, s in muts:  # a TagNop stands for one tape word: the tape keeps its length
        if name in reads:
            assert len(O.deserialize(s)[1]) == d.n
