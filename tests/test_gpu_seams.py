"""GPU: stage 1 and the whole parse with hazards exactly on the cuts of the tile plan (tests/s1_geometry.py), for every
stage-1 variant (sjhip_stage1_set_variant) and the leads 0, 1 and 63 of a device pointer.

(a) the mirror of s1_plan gives the tile count sjhip_stage1_trace reports, on every branch of the plan;
(b) stage-1 positions equal the oracle's with every hazard at every shift on every seam class, plain and ND;
(c) - (e) the whole parse (default variant) of the same documents: Tape and Strings.B equal the oracle's in both copy
modes, the values equal Python's json, MarshalJSON and Serialize equal the oracle's;
(f) the whole parse of a two-round document is the oracle's whatever variant stage 1 alone is set to."""
import concurrent.futures as cf
import contextlib
import ctypes as C
import json

import numpy as np
import pytest

import oracle_lib as O
import s1_geometry as G
import tape_reader
from test_fuzz_corpus import _same
from test_gpu_parse import check, ctx  # noqa: F401

pytestmark = pytest.mark.gpu

LEADS = (0, 1, 63)
VARIANTS = range(len(G.S1_VARIANTS))
LEAD_SETS = ((0, (0, 1)), (63, (63,)))  # documents built for lead 0 serve lead 1 too (SHIFTS reaches -3)


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def lib():
    import sjhip
    return sjhip.lib()


@contextlib.contextmanager
def variant(lib, v):
    assert lib.sjhip_stage1_set_variant(v) == v
    try:
        yield
    finally:
        lib.sjhip_stage1_set_variant(-1)  # process-global: back to the default even when the test fails


@pytest.fixture(scope="module")
def dev(cus):
    """one device buffer for every message (64 bytes of room in front for the lead) and one for the positions"""
    import torch
    n = max(G.seam_doc_length(cus), 2 * G.per_tile(0) * G.slots(0, cus) * G.UNIT + 4096) + 8192
    return torch.full((n,), 0x20, dtype=torch.uint8, device="cuda:0"), torch.empty(n // 2, dtype=torch.int32, device="cuda:0")


def _upload(buf, a, lead):
    import torch
    buf[lead:lead + a.size].copy_(torch.from_numpy(a))


def _stage1_every_variant(ctx, lib, dev, a, lead, nd, want_ok, want_pos, what, variants=VARIANTS):
    """stage 1 of a (already at buf + lead) under every variant: verdict and positions equal the oracle's"""
    import torch
    buf, pos = dev
    want = torch.from_numpy(want_pos.view(np.int32)).to("cuda:0") if want_ok else None
    for v in variants:
        with variant(lib, v):
            ok, n = ctx.stage1_device(buf.data_ptr() + lead, a.size, pos.data_ptr(), pos.numel(), ndjson=nd)
        assert ok == want_ok, (what, v, lead, nd)
        if want_ok:
            assert n == want_pos.size, (what, v, lead, nd, n, want_pos.size)
            if not torch.equal(pos[:n], want):
                got = pos[:n].cpu().numpy().view(np.uint32)
                d = np.nonzero(got != want_pos)[0]
                raise AssertionError((what, v, lead, nd, "positions differ at", d[:5], got[d[:3]], want_pos[d[:3]]))


def _with_oracle(jobs, workers=6):
    """(key, build) -> yields (key, doc, ok, positions): documents built and indexed by the oracle on a few threads
    ahead of the device (the oracle's ctypes calls run without the GIL)"""
    def run(job):
        key, build = job
        a = build()
        ok, pos = O.stage1(a, key[-1])
        return key, a, ok, pos

    jobs = list(jobs)
    with cf.ThreadPoolExecutor(max_workers=workers) as ex:
        futs = [ex.submit(run, j) for j in jobs[:workers + 1]]
        for i in range(len(jobs)):
            if i + workers + 1 < len(jobs):
                futs.append(ex.submit(run, jobs[i + workers + 1]))
            yield futs[i].result()
            futs[i] = None


# ---- (a) ----------------------------------------------------------------------------------------------------------------
def test_plan_mirror_equals_library(ctx, lib, dev, cus):
    buf, pos = dev
    lengths = {G.seam_doc_length(cus)}
    for v in VARIANTS:
        for units in G.branch_units(v, cus).values():
            lengths |= {units * G.UNIT, (units - 1) * G.UNIT + 1}
    seen = set()
    for v in VARIANTS:
        waves = G.S1_VARIANTS[v][0] // 64
        for length in sorted(lengths):
            for lead in LEADS:
                ln = length - lead if length - lead > 0 else length
                if ln + lead > buf.numel():
                    continue
                p = G.plan(ln, lead, v, cus)
                seen.add((v, p.branch, p.one_round))
                cap = (p.tiles + 8) * waves * 8
                trace = np.zeros(cap, dtype=np.uint64)
                tiles, w, words = C.c_uint(0), C.c_int(0), C.c_int(0)
                with variant(lib, v):
                    rc = lib.sjhip_stage1_trace(ctx._h, C.c_void_p(buf.data_ptr() + lead), ln, C.c_void_p(pos.data_ptr()),
                                                pos.numel(), trace.ctypes.data, cap, C.byref(tiles), C.byref(w), C.byref(words))
                assert rc == 0, (v, ln, lead, ctx.last_error())
                assert (tiles.value, w.value) == (p.tiles, waves), (v, ln, lead, tiles.value, p)
    for v in VARIANTS:  # every branch, one round (static tiles) and several (tickets)
        assert {b for (vv, b, _) in seen if vv == v} == {"small", "fold_big_su", "rounds", "fold_few_units", "tail"}, v
        assert {o for (vv, _, o) in seen if vv == v} == {True, False}, v


# ---- (b) ----------------------------------------------------------------------------------------------------------------
def test_stage1_every_hazard_on_every_seam_every_variant(ctx, lib, dev, cus):
    """rotation documents: a hazard on every 4 KiB seam; over the documents every seam of every class carries every
    hazard at every shift (tests/test_s1_geometry.py checks that)"""
    n = len(G.combos())
    jobs = [((lead0, k, nd), (lambda lead0=lead0, k=k, nd=nd: G.byte_seam_doc(k, lead0, nd, cus)[0]))
            for lead0, _ in LEAD_SETS for k in range(n) for nd in (False, True)]
    leads = dict(LEAD_SETS)
    for (lead0, k, nd), a, ok, want in _with_oracle(jobs):
        assert ok, (lead0, k, nd)
        for lead in leads[lead0]:
            _upload(dev[0], a, lead)
            _stage1_every_variant(ctx, lib, dev, a, lead, nd, ok, want, ("rotation", k))


def test_stage1_sparse_and_error_documents(ctx, lib, dev, cus):
    """blanks over whole units in front of the seams; a control character in a string on the cuts that occur once
    per plan: stage 1 fails under every variant"""
    length = G.seam_doc_length(cus)
    jobs = []
    for lead in LEADS:
        for nd in (False, True):
            jobs.append(((lead, "sparse", nd), lambda lead=lead, nd=nd: G.sparse_doc(length, lead, VARIANTS, cus, nd=nd)[0]))
    for lead in (0, 63):
        for v in (G.DEFAULT_VARIANT, 0, 2):
            _, sm = G.seams(length, lead, v, cus)
            for cls in ("full_small", "last_tile"):
                for s in (-1, 0, 1):
                    tg = [G.Target(sm[cls][0], "control_in_string", s)]
                    jobs.append(((lead, (v, cls, s), False), lambda tg=tg: G.byte_doc(length, tg)[0]))
    for (lead, what, nd), a, ok, want in _with_oracle(jobs):
        assert ok == (what == "sparse"), what
        _upload(dev[0], a, lead)
        _stage1_every_variant(ctx, lib, dev, a, lead, nd, ok, want, what)


def _token_docs():
    out = []
    for kind in sorted(G.TOKEN_KINDS):
        for d in G.TOKEN_OFFSETS:
            for nd in (False, True):
                if kind in G.ND_ONLY and not nd:
                    continue
                out.append(((kind, d, nd), G.token_doc(kind, d, O.stage1, nd=nd)[0]))
    for depth in (4095, 4096, 4097):
        out.append((("nesting", depth, False), G.nesting_doc(depth)))
    return out


@pytest.fixture(scope="module")
def token_docs():
    return _token_docs()


def test_stage1_token_documents_every_variant(ctx, lib, dev, token_docs):
    for (kind, d, nd), data in token_docs:
        a = np.frombuffer(bytearray(data), dtype=np.uint8)  # (writable: torch.from_numpy)
        ok, want = O.stage1(a, nd)
        for lead in LEADS:
            _upload(dev[0], a, lead)
            _stage1_every_variant(ctx, lib, dev, a, lead, nd, ok, want, (kind, d))


# ---- (c) - (e) -----------------------------------------------------------------------------------------------------------
def _json_values(data, nd):
    text = bytes(data).decode("utf-8")
    if nd:
        return [json.loads(line) for line in text.split("\n") if line.strip()]
    return [json.loads(text)]


def _whole(ctx, data, nd, what, values=True):
    """(c) check() of test_gpu_parse: both copy modes bit-exact; (d) the values equal Python's json; (e) MarshalJSON and
    Serialize of the resident result equal the oracle's.  values=False: no (d) (nesting deeper than Python recurses)"""
    data = bytes(data)
    check(ctx, data, nd, what)
    ref = O.parse(data, ndjson=nd, copy_strings=True)
    assert ref.rc == 0, what
    msg = bytes(data[ref.msg_off:ref.msg_off + ref.msg_len])
    pj = ctx.parse(data, ndjson=nd, copy_strings=True, key_flags=True)
    if values:
        got = tape_reader.to_python(pj.Tape, pj.Strings, msg)
        assert _same(got, _json_values(data, nd)), what
    rc, want = O.marshal_json(ref.tape, ref.strings, msg)
    assert rc == 0 and ctx.marshal_json() == want, what
    stream = ctx.serialize()
    want_stream = O.serialize(ref.tape, ref.strings, msg, dedup=False)[0]
    assert np.array_equal(stream, want_stream), what
    rc, t2, s2, m2 = O.deserialize(stream)
    assert rc == 0, what
    if values:
        assert _same(tape_reader.to_python(t2, s2, bytes(m2)), got), what


def whole_parse_docs():
    """the rotation documents at lead 0 that put each hazard once on the seams of the default plan (every seam of a
    class carries a different hazard in each): 16 of the 96"""
    n = len(G.combos())
    return [k for k in range(0, n, len(G.SHIFTS))]


def test_whole_parse_byte_seams(ctx, cus):
    for k in whole_parse_docs():
        for nd in (False, True):
            _whole(ctx, G.byte_seam_doc(k, 0, nd, cus)[0], nd, ("byte seams", k, nd))


def test_whole_parse_sparse(ctx, cus):
    length = G.seam_doc_length(cus)
    for nd in (False, True):
        _whole(ctx, G.sparse_doc(length, 0, VARIANTS, cus, nd=nd)[0], nd, ("sparse", nd))


def test_whole_parse_error_on_the_seams(ctx, cus):
    length = G.seam_doc_length(cus)
    _, sm = G.seams(length, 0, G.DEFAULT_VARIANT, cus)
    for cls in ("full_small", "last_tile"):
        for nd in (False, True):
            a = G.byte_doc(length, [G.Target(sm[cls][0], "control_in_string", 0)], nd)[0]
            check(ctx, a, nd, ("error", cls))


def test_whole_parse_token_seams(ctx, token_docs):
    for (kind, d, nd), data in token_docs:
        _whole(ctx, data, nd, (kind, d), values=kind != "nesting")
        if not nd and kind != "nesting":
            _whole(ctx, data, True, (kind, d, "as one ND record"))


# ---- (f) ----------------------------------------------------------------------------------------------------------------
def test_whole_parse_of_two_rounds_under_every_variant(ctx, lib, dev, cus):
    """the whole parse runs the default kernel and plans for it, whatever variant stage 1 alone is set to"""
    length = 2 * G.per_tile(0) * G.slots(0, cus) * G.UNIT + 777  # two rounds of variant 0, more of 2 and 5
    a, _ = G.byte_doc(length, G.rotation_targets(length, 0, 5, cus))
    ok, want = O.stage1(a)
    assert ok
    for v in (0, 2, 5):
        assert G.plan(length, 0, v, cus).nf >= 2 * G.slots(v, cus)
        with variant(lib, v):
            check(ctx, a.tobytes(), False, ("two rounds", v))
    _upload(dev[0], a, 0)
    _stage1_every_variant(ctx, lib, dev, a, 0, False, ok, want, "two rounds")
