"""GPU: sjhip_parse_batch and sjhip_parse_batch_device (k_batch_pack and the host staging, csrc/batch_api.hip) with a document,
a separator, a '\\n' or a bad ending exactly on every cut of the work: the 16 bytes of a thread, the 4096 of a block, the fast
path and the byte loop, the descriptor search, the alignment of the 16-byte load, the 64 KiB between a staged and a directly
copied document and the 32 MiB of the pinned block.  The cases are those of tests/batch_geometry.py; tests/test_batch_geometry.py
shows on the CPU that each lies on the cut it is named for (repeated here as asserts where a case is picked by its claim).

Every case is checked like test_gpu_batch.py::test_batch_equals_parse_nd_of_packed_message: Tape and Strings.B bit-equal to the
oracle's ParseND of the packed message, as many roots as documents; a case with an invalid document fails with the code the
oracle's Parse of that document gives.  Both entry points, unless the case is for one of them."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_geometry as B
import fixtures
import oracle_lib as O
from test_gpu_batch import _roots

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def ctx():
    import sjhip
    c = sjhip.Context(0)
    yield c
    c.close()


def on_device(c):
    """the case's documents in a torch buffer of exactly the bytes they take -> (tensor, offs, lens)"""
    import torch
    if c.src:
        blob, offs = c.src
    else:
        blob = b"".join(c.docs)
        offs = np.concatenate(([0], np.cumsum([len(d) for d in c.docs])[:-1])).tolist()
    lens = [len(d) for d in c.docs]
    assert max(o + n for o, n in zip(offs, lens)) == len(blob) or c.src
    dev = torch.empty(len(blob), dtype=torch.uint8, device="cuda:0")
    dev.copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
    torch.cuda.synchronize()
    return dev, offs, lens


def run(ctx, c, entry):
    if entry == "host":
        pj = ctx.parse_batch(c.docs)
        return pj.Tape, pj.Strings
    dev, offs, lens = on_device(c)
    tl, sl = ctx.parse_batch_device(dev.data_ptr(), offs, lens)
    return ctx.fetch(tl, sl)


def entries(c):
    return ("host", "device") if c.mode == "both" else (c.mode,)


def check(ctx, c, ref=None):
    """-> {entry: (tape, strings)} of a good case"""
    import sjhip
    out = {}
    for entry in entries(c):
        if c.bad is not None:
            code = O.parse(c.docs[c.bad], ndjson=False, copy_strings=True).rc
            assert code != 0 and code == c.claim.get("code", code), c.name
            with pytest.raises(sjhip.ParseError) as e:
                run(ctx, c, entry)
            assert e.value.code == code, (c.name, entry, e.value.code, str(e.value))
            continue
        r = ref or O.parse(B.packed(c.docs, entry == "host"), ndjson=True, copy_strings=True)
        assert r.rc == 0, c.name
        tape, strings = run(ctx, c, entry)
        assert np.array_equal(tape, r.tape), (c.name, entry, "tape", first_difference(tape, r.tape))
        assert np.array_equal(strings, r.strings), (c.name, entry, "Strings.B", first_difference(strings, r.strings))
        assert len(_roots(tape)) == len(c.docs), (c.name, entry)
        out[entry] = (tape, strings)
    return out


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(a[:n] != b[:n])[0]
    k = int(d[0]) if d.size else n
    return len(a), len(b), k, a[max(0, k - 4):k + 4].tolist(), b[max(0, k - 4):k + 4].tolist()


def good_batch_still_parses(ctx):
    import torch
    ref = O.parse(B.packed(B.GOOD_BATCH, False), ndjson=True, copy_strings=True)
    c = B.case("good", B.GOOD_BATCH)
    for entry in ("host", "device"):
        tape, strings = run(ctx, c, entry)
        assert ref.rc == 0 and np.array_equal(tape, ref.tape) and np.array_equal(strings, ref.strings) and len(_roots(tape)) == 3
    del torch


# ---- chunk and block cuts -----------------------------------------------------------------------------------------------------------
CUTS = B.cuts()


@pytest.mark.parametrize("i", range(len(CUTS)), ids=[c.name for c in CUTS])
def test_cut(ctx, i):
    c = CUTS[i]
    lens = B.lens_of(c)
    if "end" in c.claim:  # (the placement, as tests/test_batch_geometry.py checks it)
        k, off, path = c.claim["end"]
        x = B.end_owner(lens, k)
        assert x.path == path and (x.p0 + off) == sum(lens[:k + 1]) + k - 1
    if "many" in c.claim:
        assert max(len(x.docs) for x in B.chunk_paths(lens)) >= 6
    if "total" in c.claim:
        assert B.descriptors(lens)[1] == c.claim["total"] and len(lens) == c.claim["n"]
    assert c.mode == "both"
    check(ctx, c)


ALIGN = B.alignments()


@pytest.mark.parametrize("i", range(len(ALIGN)), ids=[c.name for c in ALIGN])
def test_source_alignment_and_tight_buffers(ctx, i):
    c = ALIGN[i]
    dev, offs, lens = on_device(c)
    assert dev.data_ptr() % 16 == 0 and dev.numel() == max(o + n for o, n in zip(offs, lens))  # nothing behind the last document
    if "align" in c.claim:
        desc, _ = B.descriptors(lens)
        assert all((o - d) % 16 == c.claim["align"] for o, (d, _) in zip(offs, desc))
        assert sum(x.path == B.FAST for x in B.chunk_paths(lens)) >= len(lens)
    check(ctx, c)


TRIMS = B.trims()


@pytest.mark.parametrize("i", range(len(TRIMS)), ids=[c.name for c in TRIMS])
def test_host_trims_whitespace_and_shifts_nothing(ctx, i):
    c = TRIMS[i]
    assert c.mode == "host" and B.lens_of(c, True) == [10, 33, 16]
    got = check(ctx, c)["host"]
    plain = O.parse(B.packed([d.strip(B.TRIM) for d in c.docs], False), ndjson=True, copy_strings=True)
    assert np.array_equal(got[0], plain.tape) and np.array_equal(got[1], plain.strings)


# ---- newline translation ------------------------------------------------------------------------------------------------------------
NEWLINES = B.newlines()


@pytest.mark.parametrize("i", range(len(NEWLINES)), ids=[c.name for c in NEWLINES])
def test_newline(ctx, i):
    c = NEWLINES[i]
    k, p, path = c.claim["nl"]
    assert b"\n".join(c.docs)[p] == 0x0A and B.chunk_paths(B.lens_of(c))[p // 16].path == path
    got = check(ctx, c)
    if c.claim.get("keep"):
        assert all(c.claim["keep"] in s.tobytes() for _, s in got.values()) and len(got) == 2
    if c.bad is not None:
        good_batch_still_parses(ctx)


# ---- the end check of the device call -----------------------------------------------------------------------------------------------
ENDS = B.end_checks()


@pytest.mark.parametrize("i", range(len(ENDS)), ids=[c.name for c in ENDS])
def test_device_end_check(ctx, i):
    c = ENDS[i]
    x = B.end_owner(B.lens_of(c), c.bad)
    place = c.claim["place"]
    assert c.mode == "device" and c.claim["code"] == 1
    assert (place != "fast" or x.path == B.FAST) and (place != "loop" or x.path == B.LOOP)
    assert (place != "block start" or (x.p0 % 4096 == 0 and x.p0 > 0)) and (place != "last chunk" or x.p1 == B.descriptors(B.lens_of(c))[1])
    check(ctx, c)
    good_batch_still_parses(ctx)


WALKS = B.end_walks()


@pytest.mark.parametrize("i", range(len(WALKS)), ids=[c.name for c in WALKS])
def test_device_end_check_walks_back_over_whitespace(ctx, i):
    c = WALKS[i]
    check(ctx, c)
    if c.bad is not None:
        good_batch_still_parses(ctx)


# ---- host staging -------------------------------------------------------------------------------------------------------------------
STAGE = B.staging_small()


@pytest.mark.parametrize("i", range(len(STAGE)), ids=[c.name for c in STAGE])
def test_staged_and_direct_documents_alternate(ctx, i):
    c = STAGE[i]
    p = B.stage_plan(B.lens_of(c))
    assert p.copies == B.staged_runs(B.lens_of(c)) and not p.waits
    assert len(p.copies) == (1 if c.claim["big"] < B.STAGE_DOC else 3)
    check(ctx, c)


@functools.lru_cache(maxsize=None)
def filler(n, seed):
    return B.doc(n, seed)


def big_docs(lens):
    """documents of these lengths; the fillers (one string each, the cheapest text to parse) are built once per module"""
    return [filler(n, 1000 * k) for k, n in enumerate(lens)]


@pytest.mark.parametrize("delta", [0, -1, 1])
def test_pinned_block_at_the_cap(ctx, delta):
    lens = B.cap_lens(delta)
    p = B.stage_plan(lens)
    k = len(lens) - 2
    assert B.staged_need(lens[:k + 1]) == B.STAGE_CAP + delta
    if delta == 1:  # the wait happened exactly once, and the run that follows starts at stage_used == 0
        assert len(p.waits) == 1 and p.waits[0][0] == k and p.stage_at == [0, 0]
    else:           # the document still fits; the 10 bytes behind it do not
        assert p.waits == [(k + 1, B.STAGE_CAP + delta)] and p.stage_at == [0, 0]
    check(ctx, B.case("cap %+d" % delta, big_docs(lens), mode="host"))


def test_pinned_block_fills_twice_around_a_direct_copy(ctx):
    lens = B.twice_lens()
    p = B.stage_plan(lens)
    direct = next(k for k, n in enumerate(lens) if n >= B.STAGE_DOC)
    assert len(p.waits) == 2 and p.waits[0][0] < direct < p.waits[1][0]
    check(ctx, B.case("twice", big_docs(lens), mode="host"))


# ---- sequencing ---------------------------------------------------------------------------------------------------------------------
def test_seam_small_plain_seam_on_one_context(ctx):
    """the pinned block, the descriptors' arena and the packed message are reused: nothing of an earlier batch may survive"""
    seam = B.case("seq", B.docs_of([10, B.STAGE_DOC, 10, 15, 17, B.STAGE_DOC - 1, 16, 33], seed=5))
    small = B.case("seq small", B.docs_of([9, 9, 9, 40], seed=77))
    first = check(ctx, seam)
    check(ctx, small)
    one = fixtures.load("twitter")
    pj = ctx.parse(one, copy_strings=True)
    r = O.parse(one, copy_strings=True)
    assert np.array_equal(pj.Tape, r.tape) and np.array_equal(pj.Strings, r.strings)
    again = check(ctx, seam)
    for entry in ("host", "device"):
        assert np.array_equal(first[entry][0], again[entry][0]) and np.array_equal(first[entry][1], again[entry][1])


# ---- the same on the bounds-checked build -------------------------------------------------------------------------------------------
CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import torch
torch.cuda.init()
import sjhip
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
import test_gpu_batch_seams as T
ctx = sjhip.Context(0)
n = 0
for cases in (T.CUTS, T.ALIGN, T.NEWLINES, T.ENDS, T.WALKS, T.STAGE[:2]):
    for c in cases:
        T.check(ctx, c)
        n += 1
T.good_batch_still_parses(ctx)
print('ok %%d' %% n)
"""


def run_on_debug_build(debug_lib, timeout=600):
    """the chunk, block, newline and end-check cases and one staging pair in their own interpreter on the bounds-checked library:
    the oracle's results and no recorded violation (a violation fails the call with "bounds check: ...")"""
    code = CHILD % (os.path.join(ROOT, "simdjson-go_amd"), HERE)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SJHIP_LIB=debug_lib), capture_output=True, text=True,
                       timeout=timeout)
    n = len(CUTS) + len(ALIGN) + len(NEWLINES) + len(ENDS) + len(WALKS) + 2
    out = r.stdout.strip().splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok %d" % n, (r.returncode, r.stdout[-500:], r.stderr[-2500:])
