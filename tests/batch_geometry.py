"""Where the batch (sjhip_parse_batch / sjhip_parse_batch_device, csrc/batch_api.hip) cuts its work, and documents that lie on
those cuts.  No GPU import, no oracle import.

The definition: the batch is ParseND of the packed message -- packed() below: the documents (trimmed like bytes.TrimSpace for
the host call, as they are for the device call) with '\\n' inside a document turned into '\\r', joined by '\\n'.

The cuts (pinned to the source text by tests/test_batch_geometry.py):
  * k_batch_pack gives a thread CHUNK packed bytes and a block BLOCK.  A chunk of CHUNK bytes that lies inside one document takes
    the fast path (one 16-byte load, newlines_to_cr on four words, one 16-byte store; the end check only if the document ends
    with the chunk); every other chunk -- one that holds a separator or a document's start, and the short last one -- takes the
    byte loop.  chunk_paths() says for every chunk which path, which documents, which ends, which separators.
  * the host call gathers consecutive documents shorter than STAGE_DOC in a pinned block of STAGE_CAP bytes at their packed
    offsets (the separators between them stay unwritten: the kernel's work) and copies every other document directly; a document
    that no longer fits makes it wait for the copies in flight and start again at offset 0.  stage_plan() replays that loop.

doc() builds a valid document of an exact length whose string bytes are a function of their position (a running counter in base
64, started per document), so a byte one place off or from another document shows in Strings.B.  The case lists (cuts(),
newlines(), end_checks(), trims(), alignments(), staging() ...) are what tests/test_gpu_batch_seams.py runs; each case says
which cut it is for, and tests/test_batch_geometry.py checks the claim with chunk_paths() / stage_plan()."""
import collections

import numpy as np

CHUNK, BLOCK = 16, 4096
STAGE_DOC, STAGE_CAP = 64 << 10, 32 << 20
FAST, LOOP = "fast", "loop"
TRIM = b" \t\n\v\f\r"   # what bytes.TrimSpace takes off among ASCII
JSON_WS = b" \t\n\r"    # what doc_end_ok walks over
B64 = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_", dtype=np.uint8)


# ---- the definition -----------------------------------------------------------------------------------------------------------------
def packed(docs, trim):
    return b"\n".join((bytes(d).strip(TRIM) if trim else bytes(d)).replace(b"\n", b"\r") for d in docs)


def descriptors(lens):
    """-> ([(dst, len)], total): the separator behind every document but the last"""
    out, total = [], 0
    for k, ln in enumerate(lens):
        out.append((total, ln))
        total += ln + (1 if k + 1 < len(lens) else 0)
    return out, total


Chunk = collections.namedtuple("Chunk", "p0 p1 path first docs ends seps")
# first: the document doc_of finds for p0 (the one whose byte or whose separator p0 is); docs: the documents with a byte in the
# chunk; ends: those whose last byte is in it; seps: the chunk offsets of the separators in it


def chunk_paths(lens):
    desc, total = descriptors(lens)
    dsts = np.array([d for d, _ in desc], dtype=np.int64)
    out = []
    for p0 in range(0, total, CHUNK):
        p1 = min(p0 + CHUNK, total)
        k = int(np.searchsorted(dsts, p0, side="right")) - 1
        dst, ln = desc[k]
        path = FAST if (p1 <= dst + ln and p0 + CHUNK == p1) else LOOP
        docs, ends, seps = [], [], []
        j = k
        while j < len(desc) and desc[j][0] < p1:
            a, b = desc[j][0], desc[j][0] + desc[j][1]  # content [a, b), separator at b
            if max(a, p0) < min(b, p1):
                docs.append(j)
            if p0 <= b - 1 < p1:
                ends.append(j)
            if j + 1 < len(desc) and p0 <= b < p1:
                seps.append(b - p0)
            j += 1
        out.append(Chunk(p0, p1, path, k, tuple(docs), tuple(ends), tuple(seps)))
    return out


def end_owner(lens, k):
    """the chunk that owns the last byte of document k"""
    desc, _ = descriptors(lens)
    return chunk_paths(lens)[(desc[k][0] + desc[k][1] - 1) // CHUNK]


Plan = collections.namedtuple("Plan", "copies stage_at waits tail")
# copies: (dst, bytes, staged?) in issue order; stage_at: the block offset a staged copy reads from (None: direct);
# waits: (document, stage_used when the block was found full, after the flush); tail: stage_used + run_len behind the last document


def stage_plan(lens, stage_doc=STAGE_DOC, stage_cap=STAGE_CAP):
    desc, _ = descriptors(lens)
    copies, stage_at, waits = [], [], []
    run_dst = run_len = stage_used = 0

    def flush():
        nonlocal run_len, stage_used
        if run_len:
            copies.append((run_dst, run_len, True))
            stage_at.append(stage_used)
        stage_used += run_len
        run_len = 0

    for k, (dst, ln) in enumerate(desc):
        if ln >= stage_doc:
            flush()
            copies.append((dst, ln, False))
            stage_at.append(None)
            continue
        gap = dst - (run_dst + run_len) if run_len else 0
        if stage_used + run_len + gap + ln > stage_cap:
            flush()
            waits.append((k, stage_used))
            stage_used = 0
        if run_len == 0:
            run_dst = dst
        else:
            run_len += dst - (run_dst + run_len)
        run_len += ln
    tail = stage_used + run_len
    flush()
    return Plan(copies, stage_at, waits, tail)


def staged_runs(lens, stage_doc=STAGE_DOC):
    """the copies of a batch that never fills the block, from the definition: every maximal run of consecutive documents below
    stage_doc with the separators between them is one staged copy, every other document one direct copy"""
    desc, _ = descriptors(lens)
    out = []
    for dst, ln in desc:
        if ln >= stage_doc:
            out.append((dst, ln, False))
        elif out and out[-1][2] and out[-1][0] + out[-1][1] + 1 == dst:
            out[-1] = (out[-1][0], dst + ln - out[-1][0], True)
        else:
            out.append((dst, ln, True))
    return out


def staged_need(lens, stage_doc=STAGE_DOC, stage_cap=STAGE_CAP):
    """stage_used + run_len + gap + len as the host loop computes it for the LAST document (which must be a staged one)"""
    assert lens[-1] < stage_doc
    p = stage_plan(lens[:-1], stage_doc, stage_cap)
    open_run = bool(lens[:-1]) and lens[-2] < stage_doc and p.tail > 0
    # (the run is open iff the document in front was staged; a wait in front of it leaves an open run too)
    return p.tail + (1 if open_run else 0) + lens[-1]


# ---- documents ----------------------------------------------------------------------------------------------------------------------
def doc(n, seed=0, ws=None, lead=b"", trail=b"", utf8=(), raw=None, empty=b"[]"):
    """A valid document of exactly n >= 2 bytes (without lead / trail): '[' ... ']' holding strings (and digits where a single
    byte is left), the first value bare, every later one behind a ',' that starts its run.
      ws:    {offset: whitespace byte} between the tokens;  lead / trail: whitespace around the document
      utf8:  offsets at which the two bytes of U+010A (c4 8a) stand inside a string
      raw:   {offset: byte} written last, whatever it breaks (a '\\n' inside a string)
    A string byte at offset i is B64[(seed + i) % 64]."""
    assert n >= 2
    if n == 2 and not ws:
        return bytes(lead) + empty + bytes(trail)
    ws = dict(ws or {})
    assert all(0 < o < n - 1 and bytes([b]) in (b" ", b"\t", b"\n", b"\r") for o, b in ws.items()), ws
    a = B64[(seed + np.arange(n)) % 64].copy()
    a[0], a[n - 1] = ord("["), ord("]")
    for o, b in ws.items():
        a[o] = b
    first = True
    i = 1
    while i < n - 1:
        if i in ws:
            i += 1
            continue
        j = min((o for o in ws if o > i), default=n - 1)
        m = j - i  # a run of m bytes between whitespace
        if not first:
            assert m >= 2, ("a run behind the first needs a ',' and a value", i, m)
            a[i] = ord(",")
            i, m = i + 1, m - 1
        first = False
        if m == 1:
            a[i] = ord("0") + (seed + i) % 10
        else:
            a[i] = a[i + m - 1] = ord('"')
        i = j
    for o in utf8:
        assert a[o] in B64 and a[o + 1] in B64 and 0 < o < n - 2, o
        a[o], a[o + 1] = 0xC4, 0x8A
    for o, b in (raw or {}).items():
        a[o] = b
    return bytes(lead) + a.tobytes() + bytes(trail)


def docs_of(lens, seed=0):
    """documents of these lengths; '[]' and '{}' alternate among the two-byte ones"""
    return [doc(n, seed + 1000 * k, empty=b"{}" if k % 2 else b"[]") for k, n in enumerate(lens)]


def ws_of(n, nl_every=3):
    """n whitespace bytes with '\\n' among them"""
    return bytes(b" \t\r\n"[(3 if k % nl_every == 0 else k) % 4] for k in range(n))


Case = collections.namedtuple("Case", "name docs mode bad claim src")
# mode: "both", "host" or "device"; bad: None, or the index of the one invalid document; claim: what test_batch_geometry checks
# (a dict, by family); src: None (the device buffer is the documents back to back, nothing behind the last) or (blob, offs)


def case(name, docs, mode="both", bad=None, claim=None, src=None):
    return Case(name, list(docs), mode, bad, claim or {}, src)


def lens_of(c, trim=False):
    return [len(bytes(d).strip(TRIM)) if trim else len(d) for d in c.docs]


# ---- chunk and block cuts -----------------------------------------------------------------------------------------------------------
SIZES = (2, 3, 15, 16, 17, 31, 32, 33)


def cuts():
    out = []

    def add(name, lens, **claim):
        out.append(case("cut " + name, docs_of(lens, seed=len(out)), claim=dict(claim, lens=list(lens))))

    # a document's last byte at chunk offset 15 (fast path, end check), 14 and 0 (byte loop); its separator at 0, 15 and 1
    add("end at 15 fast", [16, 20], end=(0, 15, FAST), sep=[(0, 16 % CHUNK)])
    add("end at 15 fast, deep", [48, 20], end=(0, 15, FAST))
    add("end at 14 loop, separator at 15", [15, 20], end=(0, 14, LOOP), sep=[(0, 15)])
    add("end at 0 loop", [17, 20], end=(0, 0, LOOP), sep=[(0, 1)])
    add("end at 15 of a chunk with two documents", [5, 10, 20], end=(1, 15, LOOP))
    # the separator on the first and the last byte of a block
    add("separator at block offset 0", [4096, 20], end=(0, 15, FAST), block_sep=0)
    add("separator at block offset 4095", [4095, 20], end=(0, 14, LOOP), block_sep=4095)
    add("separator at block offset 0, behind short documents", [2000, 2095, 33], block_sep=0)
    # the lengths of the issue, every rotation (every length meets other alignments)
    for r in range(len(SIZES)):
        add("sizes rotated by %d" % r, SIZES[r:] + SIZES[:r], sizes=True)
    add("six documents in one chunk", [2] * 8, many=6)
    add("six documents in the second chunk", [17] + [2] * 9 + [3], many=6)
    add("from a separator into the third document behind it", [16, 3, 3, 20], walk=(1, 3))
    # total modulo 16 and 4096; n = 1, 2, 3
    for n in (1, 2, 3):
        for total in (32, 33, 31, 4096, 4097, 4095, 8192, 8193, 8191):
            lens = [10] * (n - 1)
            lens.append(total - 11 * (n - 1))
            add("n = %d, total %d" % (n, total), lens, total=total, n=n)
    # doc_of asked for the first document, for a separator byte of every document, and for the last document
    for n in (257, 4097):
        add("%d documents" % n, [16] + [15] * (n - 2) + [40], search=n)
    return out


# ---- newline translation ------------------------------------------------------------------------------------------------------------
def _nl_cases(out, tag, pair):
    """the whitespace bytes `pair` (holding a '\\n') in a fast-path chunk and in a byte-loop chunk, the '\\n' at every chunk offset"""
    nl = pair.index(b"\n")
    for j in range(CHUNK):
        # fast: [80, 20]: chunk 2 (bytes 32..47) lies inside the 80-byte document
        o = 32 + j - nl
        ws = {o + i: pair[i] for i in range(len(pair))}
        out.append(case("nl %s fast at %d" % (tag, j), [doc(80, 7 * j, ws=ws), doc(20, 99)], claim=dict(nl=(0, 32 + j, FAST))))
        # loop: [4, 26]: document 1 lies at 5..30 and the message has 31 bytes: chunk 0 holds a separator, chunk 1 is short.
        # The pair goes to the packed offset p = j or j + 16 that leaves document 1 valid (doc(): a run of two bytes or none behind)
        for p in (j, j + CHUNK):
            o = p - 5 - nl
            left = 24 - (o + len(pair) - 1)
            if o >= 1 and left >= 0 and left != 1:
                ws = {o + i: pair[i] for i in range(len(pair))}
                out.append(case("nl %s loop at %d" % (tag, j), [doc(4, 3), doc(26, 5 * j, ws=ws)], claim=dict(nl=(1, p, LOOP))))
                break
        else:
            raise AssertionError(("no room", tag, j))


def newlines():
    out = []
    _nl_cases(out, "alone", b"\n")
    for tag, pair in (("behind tab", b"\t\n"), ("before tab", b"\n\t"), ("behind cr", b"\r\n"), ("before cr", b"\n\r")):
        sub = []
        _nl_cases(sub, tag, pair)
        out += [c for c in sub if c.claim["nl"][1] % 4 in (0, 3) or c.claim["nl"][1] % CHUNK in (0, 15)]  # word and chunk edges
    # beside a vertical tab: 0x0b is no JSON whitespace, the document is invalid (the oracle's Parse says with which code); were
    # it turned into '\r', or the '\n' beside it left alone, the verdict would change
    for j, pth in ((5, FAST), (8, FAST)):
        d = doc(80, 11, ws={32 + j: 0x0A, 33 + j: 0x20}, raw={33 + j: 0x0B})
        out.append(case("nl before 0x0b %s at %d" % (pth, j), [d, doc(20, 1)], bad=0, claim=dict(nl=(0, 32 + j, pth))))
        d = doc(80, 12, ws={32 + j: 0x20, 33 + j: 0x0A}, raw={32 + j: 0x0B})
        out.append(case("nl behind 0x0b %s at %d" % (pth, j), [d, doc(20, 1)], bad=0, claim=dict(nl=(0, 33 + j, pth))))
    d = doc(26, 13, ws={8: 0x0A, 9: 0x20}, raw={9: 0x0B})
    out.append(case("nl before 0x0b loop", [doc(4, 3), d], bad=1, claim=dict(nl=(1, 13, LOOP))))
    # U+010A ends a string, its quote, then the '\n': 0x8a and 0x0a in one word at every byte lane; Strings.B keeps the 0x8a
    for j in range(4, 8):
        d = doc(80, 17 + j, ws={32 + j: 0x0A}, utf8=(32 + j - 3,))
        out.append(case("nl behind 0x8a fast at %d" % j, [d, doc(20, 1)], claim=dict(nl=(0, 32 + j, FAST), keep=0x8A)))
    d = doc(26, 19, ws={9: 0x0A}, utf8=(6,))
    out.append(case("nl behind 0x8a loop", [doc(4, 3), d], claim=dict(nl=(1, 14, LOOP), keep=0x8A)))
    # a raw '\n' inside a string (right behind a 0x8a): stage-1 error, from the fast path and from the byte loop
    for j in (0, 6, 15):
        d = doc(80, 23 + j, utf8=(32 + j - 2,), raw={32 + j: 0x0A})
        out.append(case("nl inside a string fast at %d" % j, [d, doc(20, 1)], bad=0, claim=dict(nl=(0, 32 + j, FAST), code=1)))
    d = doc(26, 29, utf8=(7,), raw={9: 0x0A})
    out.append(case("nl inside a string loop", [doc(4, 3), d], bad=1, claim=dict(nl=(1, 14, LOOP), code=1)))
    d = doc(20, 31, raw={9: 0x0A})
    out.append(case("nl inside a string, last short chunk", [doc(4, 3), d], bad=1, claim=dict(nl=(1, 14, LOOP), code=1)))
    return out


# ---- the end check of the device call -----------------------------------------------------------------------------------------------
BAD_ENDS = (b"1", b'"str"', b'{"a":1', b'{"a":1} x', b"[1,2", b"true", b" \t\r\n ")
PLACES = ("fast", "loop", "block start", "last chunk")


def end_checks():
    """every bad ending, its last byte owned by a fast-path chunk, a byte-loop chunk, the first chunk of a block, the last chunk
    of the message (padded in front with spaces where the place asks for length: the device call takes documents as they are)"""
    out = []
    for b, bad in enumerate(BAD_ENDS):
        for place in PLACES:
            if place == "fast":      # 10 + separator, then the document up to byte 47: chunk 2 lies inside it
                docs, k = [doc(10, b), b" " * (37 - len(bad)) + bad, doc(20, b + 1)], 1
            elif place == "loop":    # the document as it is behind a separator
                docs, k = [doc(10, b), bad, doc(40, b + 1)], 1
            elif place == "block start":  # ends at byte 4096 + 7
                docs, k = [doc(4090, b), b" " * (13 - len(bad)) + bad, doc(20, b + 1)], 1
            else:
                docs, k = [doc(10, b), doc(20, b + 1), bad], 2
            out.append(case("end %r %s" % (bad, place), docs, mode="device", bad=k, claim=dict(place=place, code=1)))
    return out


def end_walks():
    """the backwards walk of the end check across chunks and a block; all-whitespace documents of exactly a chunk and a block"""
    out = []
    for n in (17, 4096, 4097):
        out.append(case("end behind %d bytes of whitespace" % n, [doc(10, 1), doc(30, 2, trail=ws_of(n)), doc(20, 3)], mode="device",
                        claim=dict(trail=n)))
        out.append(case("end behind %d bytes of whitespace, last" % n, [doc(10, 1), doc(30, 2, trail=ws_of(n))], mode="device",
                        claim=dict(trail=n)))
    # whitespace in front of the first document: ParseND trims it off its message, the roots stay where they are
    for n in (1, 17):
        out.append(case("first document behind %d bytes of whitespace" % n, [doc(30, 2, lead=ws_of(n)), doc(20, 3)], mode="device",
                        claim=dict(lead=n)))
    for n in (16, 4096):
        # at packed offset 0 (every chunk of it on the fast path) and behind a separator
        out.append(case("all whitespace, %d bytes, first" % n, [ws_of(n), doc(20, 3)], mode="device", bad=0, claim=dict(blank=n, code=1)))
        out.append(case("all whitespace, %d bytes" % n, [doc(10, 1), ws_of(n), doc(20, 3)], mode="device", bad=1,
                        claim=dict(blank=n, code=1)))
    return out


GOOD_BATCH = [b'{"x":1}', b"[1,2,3]", b'{"k":[true,null]}']


# ---- host only: trimming ------------------------------------------------------------------------------------------------------------
TRIMS = (0, 1, 15, 16, 4097)


def trims():
    out = []
    for a in TRIMS:
        for b in TRIMS:
            docs = [doc(10, 1, lead=ws_of(b), trail=ws_of(a)), doc(33, 2, lead=ws_of(a), trail=ws_of(b)), doc(16, 3, lead=ws_of(a, 2))]
            out.append(case("trim %d / %d" % (a, b), docs, mode="host", claim=dict(trim=(a, b))))
    return out


# ---- device only: the alignment of the 16-byte load ---------------------------------------------------------------------------------
def alignments():
    """documents that take the fast path at every offs[k] - dst[k] modulo 16 (the device pointer of the buffer is aligned far
    above 16), with room between them; and back to back with nothing behind the last one, whose last chunk is a short one"""
    out = []
    lens = [40, 37, 50, 64]
    desc, _ = descriptors(lens)
    for a in range(CHUNK):
        docs = docs_of(lens, seed=a)
        blob, offs = bytearray(), []
        for (dst, ln), d in zip(desc, docs):
            blob += b"\xee" * ((dst + a - len(blob)) % CHUNK + 3 * CHUNK)  # (filler no document holds: a load from it would show)
            assert (len(blob) - dst) % CHUNK == a
            offs.append(len(blob))
            blob += d
        out.append(case("alignment %d" % a, docs, mode="device", claim=dict(align=a), src=(bytes(blob), offs)))
    for r in range(CHUNK):
        out.append(case("back to back, last document of %d bytes" % (33 + r), docs_of([40, 37, 33 + r], seed=r), mode="device",
                        claim=dict(tight=True)))
    # the same with the documents in reverse order in the buffer: the FIRST document of the batch has nothing behind it, and its
    # last chunk is a full one that runs on into the next document
    for r in (0, 7, 15):
        docs = docs_of([40 + r, 37, 50], seed=r)
        offs = [len(docs[1]) + len(docs[2]), len(docs[2]), 0]
        out.append(case("back to back in reverse, first document of %d bytes" % (40 + r), docs, mode="device",
                        claim=dict(tight=True), src=(docs[2] + docs[1] + docs[0], offs)))
    return out


# ---- host only: staging -------------------------------------------------------------------------------------------------------------
def staging_small():
    """documents of STAGE_DOC - 1, STAGE_DOC and STAGE_DOC + 1 bytes between 10-byte ones, and the other way round: staged runs and
    direct copies alternate, the separator between the two kinds is the kernel's alone"""
    out = []
    for big in (STAGE_DOC - 1, STAGE_DOC, STAGE_DOC + 1):
        for order, lens in (("small-big-small", [10, big, 10]), ("big-small-big", [big, 10, big])):
            out.append(case("stage %d %s" % (big, order), docs_of(lens, seed=big), mode="host", claim=dict(lens=lens, big=big)))
    return out


def cap_lens(delta, filler=STAGE_DOC - 1, stage_cap=STAGE_CAP):
    """lengths whose staged bytes make `stage_used + run_len + gap + len` of the last-but-one document come out at
    stage_cap + delta; a 10-byte document follows.  Worked out with stage_plan from the filler length alone."""
    n = (stage_cap - (1 << 16)) // (filler + 1)   # fillers, leaving room for two documents of about half a STAGE_DOC
    lens = [filler] * n
    half = (stage_cap - stage_plan(lens, stage_cap=stage_cap).tail - 2) // 2
    lens.append(half)
    last = stage_cap + delta - (stage_plan(lens, stage_cap=stage_cap).tail + 1)
    assert 2 <= last < STAGE_DOC and 2 <= half < STAGE_DOC, (half, last)
    lens += [last, 10]
    assert staged_need(lens[:-1], stage_cap=stage_cap) == stage_cap + delta
    return lens


def twice_lens(filler=STAGE_DOC - 1, stage_cap=STAGE_CAP):
    """the block fills, a few documents later a direct copy, then the block fills again"""
    n = stage_cap // (filler + 1) + 5
    return [filler] * n + [STAGE_DOC + 4465] + [filler] * n + [10]
