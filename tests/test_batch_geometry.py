"""CPU: tests/batch_geometry.py agrees with itself and with the source text of csrc/batch_api.hip, every case list of
tests/test_gpu_batch_seams.py lies on the cut it is named for, and sj::newlines_to_cr is the byte-wise definition on every pair of
adjacent bytes."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import batch_geometry as B
import oracle_lib as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simdjson-go_amd", "csrc")
SMALL = [f() for f in (B.cuts, B.newlines, B.end_checks, B.end_walks, B.trims, B.alignments, B.staging_small)]


def by_claim(cases, key):
    return [c for c in cases if key in c.claim]


# ---- the helper against itself ------------------------------------------------------------------------------------------------------
def test_packed_has_length_total_and_chunks_tile_it():
    for c in itertools.chain(*SMALL):
        for trim in ([True] if c.mode == "host" else [False] if c.mode == "device" else [True, False]):
            lens = B.lens_of(c, trim)
            desc, total = B.descriptors(lens)
            msg = B.packed(c.docs, trim)
            assert len(msg) == total, c.name
            for k, (dst, ln) in enumerate(desc):  # every document at its offset, a separator behind all but the last
                assert msg[dst:dst + ln] == (c.docs[k].strip(B.TRIM) if trim else c.docs[k]).replace(b"\n", b"\r"), (c.name, k)
                assert k + 1 == len(desc) or msg[dst + ln] == 0x0A
            assert msg.count(b"\n") == len(lens) - 1
            if total > 70000:
                continue
            ch = B.chunk_paths(lens)
            assert [x.p0 for x in ch] == list(range(0, total, B.CHUNK)) and ch[-1].p1 == total
            assert all(x.p1 - x.p0 == B.CHUNK for x in ch[:-1])
            assert sorted(k for x in ch for k in x.ends) == list(range(len(lens)))  # every end owned once
            assert sum(len(x.seps) for x in ch) == len(lens) - 1
            for x in ch:  # a fast chunk holds sixteen bytes of one document and no separator
                if x.path == B.FAST:
                    assert len(x.docs) == 1 and not x.seps and x.p1 - x.p0 == B.CHUNK and b"\n" not in msg[x.p0:x.p1]


def test_builder_lengths_and_position_bytes():
    for n in list(range(2, 70)) + [4095, 4096, 4097, B.STAGE_DOC - 1, B.STAGE_DOC, B.STAGE_DOC + 1]:
        d = B.doc(n, seed=n)
        assert len(d) == n and d == d.strip(B.TRIM)
        assert O.parse(d, ndjson=False, copy_strings=True).rc == 0, n
        if n > 4:
            r = O.parse(d, ndjson=False, copy_strings=True)
            assert r.strings.tobytes() == bytes(B.B64[(n + np.arange(2, n - 2)) % 64]), n
    a, b = B.doc(40, 0), B.doc(40, 1)
    assert a[3:-2] == b[2:-3]  # (a byte one place off is another byte)


def test_mirror_constants_are_the_sources():
    src = open(os.path.join(CSRC, "batch_api.hip")).read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) >= 1 and len(set(m)) == 1, (pattern, m)
        return m[0]

    m = one(r"constexpr size_t STAGE_DOC = (\d+) << (\d+), STAGE_CAP = (\d+) << (\d+);")
    assert int(m[0]) << int(m[1]) == B.STAGE_DOC and int(m[2]) << int(m[3]) == B.STAGE_CAP
    # bytes per block: the kernel's index and both launches' grids; bytes per thread: the index and the chunk end
    assert int(one(r"blockIdx\.x \* (\d+) \+")) == B.BLOCK
    assert int(one(r"threadIdx\.x \* (\d+);")) == B.CHUNK
    blk = re.findall(r"\(total \+ (\d+)\) / (\d+)\)", src)
    assert len(blk) == 2 and all(int(a) + 1 == B.BLOCK and int(b) == B.BLOCK for a, b in blk)
    assert {int(x) for x in re.findall(r"p0 \+ (\d+)", src)} == {B.CHUNK}
    assert int(one(r"__launch_bounds__\((\d+)\) void k_batch_pack")) * B.CHUNK == B.BLOCK
    assert {int(x) for x in re.findall(r"dim3\((\d+)\), 0, ctx->stream", src)} == {B.BLOCK // B.CHUNK}


# ---- every case on the branch it is named for ---------------------------------------------------------------------------------------
def test_cut_cases_lie_on_their_cuts():
    cs = B.cuts()
    seen = dict(end=set(), sep=set(), block_sep=set(), sizes=set(), mod16=set(), mod4096=set(), n=set(), many=0, walk=0, search=set())
    for c in cs:
        lens = B.lens_of(c)
        assert lens == c.claim["lens"] and B.lens_of(c, True) == lens  # (nothing to trim: both calls pack the same message)
        desc, total = B.descriptors(lens)
        ch = B.chunk_paths(lens)
        if "end" in c.claim:
            k, off, path = c.claim["end"]
            x = B.end_owner(lens, k)
            assert (desc[k][0] + desc[k][1] - 1) % B.CHUNK == off and x.path == path, c.name
            if path == B.FAST:
                assert x.p1 == desc[k][0] + desc[k][1]  # the only way the fast path runs the end check
            seen["end"].add((off, path))
        for k, off in c.claim.get("sep", []):
            assert (desc[k][0] + desc[k][1]) % B.CHUNK == off, c.name
            seen["sep"].add(off)
        if "block_sep" in c.claim:
            assert any((d + ln) % B.BLOCK == c.claim["block_sep"] for d, ln in desc[:-1]), c.name
            seen["block_sep"].add(c.claim["block_sep"])
        if "sizes" in c.claim:
            assert sorted(lens) == list(B.SIZES)
            seen["sizes"].add(tuple(d % B.CHUNK for d, _ in desc))
        if "many" in c.claim:
            assert max(len(x.docs) for x in ch) >= c.claim["many"], c.name
            seen["many"] += 1
        if "walk" in c.claim:
            x = ch[c.claim["walk"][0]]
            assert x.seps[0] == 0 and x.first == 0 and x.docs == (1, 2, 3) and 3 not in x.ends and len(x.seps) == 3, c.name
            seen["walk"] += 1
        if "total" in c.claim:
            assert total == c.claim["total"] and len(lens) == c.claim["n"]
            seen["mod16"].add((len(lens), total % B.CHUNK))
            seen["mod4096"].add((len(lens), total % B.BLOCK))
            seen["n"].add(len(lens))
            if total % B.CHUNK:
                assert ch[-1].path == B.LOOP  # the short last chunk, inside one document for n = 1 and n = 2
                assert len(lens) == 3 or (ch[-1].docs == (len(lens) - 1,) and not ch[-1].seps)
        if "search" in c.claim:
            n = c.claim["search"]
            firsts = [x.first for x in ch]
            assert len(lens) == n and firsts[0] == 0 and firsts[-1] == n - 1
            seps = {d + ln for d, ln in desc[:-1]}
            assert all(x.p0 in seps for x in ch[1:n]) and sorted(set(firsts)) == list(range(n))  # (and every one between)
            seen["search"].add(n)
    assert seen["end"] >= {(15, B.FAST), (14, B.LOOP), (0, B.LOOP), (15, B.LOOP)}
    assert seen["sep"] >= {0, 15} and seen["block_sep"] == {0, 4095}
    assert len(seen["sizes"]) == len(B.SIZES) and seen["many"] == 2 and seen["walk"] == 1
    assert seen["n"] == {1, 2, 3} and seen["search"] == {257, 4097}
    for n in (1, 2, 3):
        assert {m for k, m in seen["mod16"] if k == n} >= {0, 1, 15} and {m for k, m in seen["mod4096"] if k == n} >= {0, 1, 4095}


def test_newline_cases_lie_on_their_paths():
    cs = B.newlines()
    alone = {B.FAST: set(), B.LOOP: set()}
    beside = {0x09: set(), 0x0D: set(), 0x0B: set(), 0x8A: set()}
    inside = set()
    for c in cs:
        k, p, path = c.claim["nl"]
        lens = B.lens_of(c)
        desc, _ = B.descriptors(lens)
        raw = b"\n".join(c.docs)  # before translation
        assert raw[p] == 0x0A and desc[k][0] < p < desc[k][0] + desc[k][1] - 1, c.name
        assert B.chunk_paths(lens)[p // B.CHUNK].path == path, c.name
        assert B.packed(c.docs, False)[p] == 0x0D
        one = O.parse(c.docs[k], ndjson=False, copy_strings=True)
        if c.bad is None:
            assert all(O.parse(d, ndjson=False, copy_strings=True).rc == 0 for d in c.docs), c.name
        else:
            assert c.bad == k and one.rc != 0 and one.rc == c.claim.get("code", one.rc), (c.name, one.rc)
            assert all(O.parse(d, ndjson=False, copy_strings=True).rc == 0 for j, d in enumerate(c.docs) if j != k), c.name
        if " alone " in c.name:
            alone[path].add(p % B.CHUNK)
        for b in beside:
            if b in (raw[p - 1], raw[p + 1]) or (b == 0x8A and raw[p - 2] == b):
                beside[b].add(path)
        if c.claim.get("keep"):
            r = O.parse(B.packed(c.docs, False), ndjson=True, copy_strings=True)
            assert r.rc == 0 and 0x8A in r.strings.tobytes(), c.name
        if "inside a string" in c.name:
            assert one.rc == 1
            inside.add(path)
    assert alone[B.FAST] == set(range(B.CHUNK)) and alone[B.LOOP] == set(range(B.CHUNK))
    assert all(v == {B.FAST, B.LOOP} for v in beside.values()), beside
    assert inside == {B.FAST, B.LOOP}


def test_end_check_cases_lie_on_their_places():
    cs = B.end_checks()
    assert len(cs) == len(B.BAD_ENDS) * len(B.PLACES)
    seen = set()
    for c in cs:
        lens = B.lens_of(c)
        bad = c.docs[c.bad]
        which, = [b for b in B.BAD_ENDS if bad.endswith(b) and not bad[:len(bad) - len(b)].strip(b" ")]
        assert O.parse(bad, ndjson=False, copy_strings=True).rc == 1, c.name
        assert all(O.parse(d, ndjson=False, copy_strings=True).rc == 0 for j, d in enumerate(c.docs) if j != c.bad)
        x = B.end_owner(lens, c.bad)
        ch = B.chunk_paths(lens)
        place = c.claim["place"]
        if place == "fast":
            assert x.path == B.FAST and x.ends == (c.bad,)
        elif place == "loop":
            assert x.path == B.LOOP
        elif place == "block start":
            assert x.p0 % B.BLOCK == 0 and x.p0 > 0
        else:
            assert x is ch[-1] or x == ch[-1]
        seen.add((which, place))
    assert len(seen) == len(cs)
    for c in B.end_walks():
        lens = B.lens_of(c)
        if "trail" in c.claim:
            n = c.claim["trail"]
            d = c.docs[1]
            assert len(d) == 30 + n and d[:30].endswith(b"]") and not d[30:].strip(B.JSON_WS) and b"\n" in d[30:]
            assert all(O.parse(d, ndjson=False, copy_strings=True).rc == 0 for d in c.docs)
            assert (B.descriptors(lens)[0][1][0] + 30) // B.CHUNK < (B.descriptors(lens)[0][1][0] + len(d) - 1) // B.CHUNK
        elif "lead" in c.claim:
            n = c.claim["lead"]
            assert len(c.docs[0]) == 30 + n and not c.docs[0][:n].strip(B.JSON_WS) and c.docs[0][n:n + 1] == b"["
        else:
            d = c.docs[c.bad]
            assert len(d) == c.claim["blank"] and not d.strip(B.JSON_WS) and O.parse(d, ndjson=False, copy_strings=True).rc == 1
            if c.bad == 0:
                assert all(x.path == B.FAST for x in B.chunk_paths(lens)[:len(d) // B.CHUNK])


def test_trim_alignment_and_staging_cases():
    for c in B.trims():
        a, b = c.claim["trim"]
        assert [len(d) for d in c.docs] == [10 + a + b, 33 + a + b, 16 + a] and B.lens_of(c, True) == [10, 33, 16]
        assert a == 0 or any(b"\n" in d[:a] for d in c.docs)
    assert {c.claim["trim"] for c in B.trims()} == set(itertools.product(B.TRIMS, B.TRIMS))
    aligns = set()
    for c in B.alignments():
        lens = B.lens_of(c)
        desc, _ = B.descriptors(lens)
        ch = B.chunk_paths(lens)
        if "align" in c.claim:
            blob, offs = c.src
            for k, (dst, ln) in enumerate(desc):
                assert blob[offs[k]:offs[k] + ln] == c.docs[k] and (offs[k] - dst) % B.CHUNK == c.claim["align"]
                assert any(x.path == B.FAST and x.docs == (k,) for x in ch), (c.name, k)
            aligns.add(c.claim["align"])
        elif c.src:
            blob, offs = c.src
            x = B.end_owner(lens, 0)  # nothing behind document 0 in the buffer, and a full chunk runs on past its end
            assert offs[0] + lens[0] == len(blob) and x.p1 - x.p0 == B.CHUNK and x.p1 > lens[0] and x.path == B.LOOP
        else:
            assert ch[-1].path == B.LOOP or ch[-1].ends == (len(lens) - 1,)
    assert aligns == set(range(B.CHUNK))
    for c in B.staging_small():
        lens = B.lens_of(c)
        p = B.stage_plan(lens)
        assert B.staged_runs(lens) == p.copies and not p.waits, c.name
        assert len(p.copies) == (1 if c.claim["big"] < B.STAGE_DOC else 3)  # one run, or runs and direct copies in turn
    assert {(c.claim["big"] - B.STAGE_DOC) for c in B.staging_small()} == {-1, 0, 1}


def test_stage_plan_at_the_cap():
    """the cap arithmetic needs only the lengths"""
    for delta in (-1, 0, 1):
        lens = B.cap_lens(delta)
        p = B.stage_plan(lens)
        k = len(lens) - 2  # the document that brings the block to cap + delta
        assert B.staged_need(lens[:k + 1]) == B.STAGE_CAP + delta
        if delta <= 0:  # it still fits (exactly, for 0); the 10-byte document behind it is the one that waits
            assert p.waits == [(k + 1, B.STAGE_CAP + delta)]
        else:           # it waits, exactly once, and the run that follows starts at offset 0 of the block
            assert p.waits == [(k, p.copies[0][1])] and len(p.waits) == 1
        assert [st for _, _, st in p.copies] == [True, True] and p.stage_at == [0, 0]
        assert sum(n for _, n, _ in p.copies) + 1 == B.descriptors(lens)[1]
    lens = B.twice_lens()
    p = B.stage_plan(lens)
    direct = next(k for k, ln in enumerate(lens) if ln >= B.STAGE_DOC)
    assert len(p.waits) == 2 and p.waits[0][0] < direct < p.waits[1][0]
    assert [st for _, _, st in p.copies] == [True, True, False, True, True] and p.stage_at[3] > 0 and p.stage_at[4] == 0
    # a small block, by hand: 3 + 1 + 3 fill a block of 7; the third document waits and starts at 0; the direct copy closes its
    # run (3 bytes in flight); 2 more fit behind them, the separator and the last 2 do not
    p = B.stage_plan([3, 3, 3, 9, 2, 2], stage_doc=8, stage_cap=7)
    assert p.copies == [(0, 7, True), (8, 3, True), (12, 9, False), (22, 2, True), (25, 2, True)]
    assert p.stage_at == [0, 0, None, 3, 0] and p.waits == [(2, 7), (5, 5)] and p.tail == 2


# ---- sj::newlines_to_cr -------------------------------------------------------------------------------------------------------------
def test_newlines_to_cr_on_every_pair_of_adjacent_bytes():
    import __graft_entry__ as G
    L = C.CDLL(G.build_selftest())
    L.sj_selftest_newlines_to_cr_words.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.sj_selftest_newlines_to_cr_words.restype = None
    others = np.array([0x00, 0x0A, 0x7F, 0x80, 0xFF], dtype=np.uint32)
    a, b = np.meshgrid(np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32), indexing="ij")
    a, b = a.ravel(), b.ravel()
    words = []
    for lane in range(3):  # the pair in bytes (lane, lane + 1), the other two bytes from `others`
        rest = [k for k in range(4) if k not in (lane, lane + 1)]
        for x in others:
            for y in others:
                words.append((a << np.uint32(8 * lane)) | (b << np.uint32(8 * (lane + 1))) | (x << np.uint32(8 * rest[0])) | (y << np.uint32(8 * rest[1])))
    w = np.ascontiguousarray(np.concatenate(words), dtype=np.uint32)
    assert w.size == 3 * 25 * 65536
    out = np.empty_like(w)
    L.sj_selftest_newlines_to_cr_words(w.ctypes.data, out.ctypes.data, w.size)
    by = w.view(np.uint8).copy()
    by[by == 0x0A] = 0x0D
    assert np.array_equal(out.view(np.uint8), by)
