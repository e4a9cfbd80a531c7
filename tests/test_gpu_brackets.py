"""GPU: stage 2's bracket matcher -- the tile matcher of k_s2_emit_planes, the min tree (tree12_body, k_min_upper) and
k_br_match / wave_psv_tree -- on the documents of tests/s2_brackets.py, which put a question on every group, window, level
and tile edge of it (tests/test_s2_brackets.py shows on the CPU that they do).  The verdict is the oracle's: Tape and
Strings.B bit for bit in both copy modes, its MarshalJSON text (which walks the container words), its error code."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle_lib as O
import s2_brackets as B
from test_gpu_parse import check, ctx, gpu_parse  # noqa: F401  (ctx is the module fixture)

pytestmark = pytest.mark.gpu

VALID = B.valid_docs()
ERRORS = B.error_docs()


@pytest.fixture(scope="module", autouse=True)
def torch_before_the_library():
    """PyTorch (device buffers of the pointer test) must initialise its HIP runtime before libsjhip.so brings the system's
    (tests/conftest.py does this for -m gpu runs; this keeps the file passing when it is run by name)"""
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()


def check_marshal(ctx, doc, nd, what):
    ref = O.parse(doc, ndjson=nd)
    assert ref.rc == 0, what
    rc, want = O.marshal_json(ref.tape, ref.strings, doc[ref.msg_off:ref.msg_off + ref.msg_len])
    assert rc == 0, what
    pj = ctx.parse(doc, ndjson=nd)
    assert np.array_equal(pj.Tape, ref.tape), what
    got = ctx.marshal_json()
    if got != want:
        k = next(i for i in range(min(len(got), len(want)) + 1) if got[i:i + 1] != want[i:i + 1])
        raise AssertionError((what, len(got), len(want), k, got[max(0, k - 30):k + 30], want[max(0, k - 30):k + 30]))


@pytest.mark.parametrize("name", sorted(VALID))
def test_valid_document(ctx, name):
    doc, nd = VALID[name]
    assert O.parse(doc, ndjson=nd).rc == 0
    check(ctx, doc, nd=nd, what=name)
    check_marshal(ctx, doc, nd, name)


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_error_document(ctx, name):
    doc = ERRORS[name]
    assert O.parse(doc).rc != 0
    check(ctx, doc, what=name)                       # the oracle's code in both copy modes
    twin, nd = VALID["far_nested"]
    check(ctx, twin, nd=nd, what="after " + name)    # and the context is none the worse for it


def test_nd_text_as_a_plain_document(ctx):
    """the records of long_record_nd without the ND flag: whatever the oracle says to several roots in one document"""
    check(ctx, VALID["long_records_nd"][0], nd=False, what="nd text, plain")


@pytest.mark.parametrize("lead", [1, 63])
def test_long_records_from_an_unaligned_device_pointer(ctx, lead):
    """tape_base and every offset shift with the pointer's place in its 64-byte line; the root words of the long records are
    16-byte stores at odd and even tape offsets"""
    import torch
    for name, nd in (("long_records_nd", True), ("long_records_plain", False), ("staircase", False)):
        doc = VALID[name][0]
        dev = torch.zeros(len(doc) + 512, dtype=torch.uint8, device="cuda:0")
        dev[lead:lead + len(doc)].copy_(torch.frombuffer(bytearray(doc), dtype=torch.uint8))
        torch.cuda.synchronize()
        for copy in (True, False):
            ref = O.parse(doc, ndjson=nd, copy_strings=copy)
            assert ref.rc == 0 and ref.msg_off == 0 and ref.msg_len == len(doc)
            tl, sl = ctx.parse_device(dev.data_ptr() + lead, len(doc), ndjson=nd, copy_strings=copy)
            tape, strings = ctx.fetch(tl, sl)
            assert np.array_equal(tape, ref.tape), (name, lead, copy)
            assert np.array_equal(strings, ref.strings), (name, lead, copy)


@pytest.mark.parametrize("big,small", [("far3_arr_obj", "far_a63_obj"), ("count_262146", "count_4098"),
                                       ("count_4160", "count_66"), ("staircase", "seam_a64_arr"),
                                       ("levels_both4", "levels_host4_device3")])
def test_alternating_sizes_on_one_context(ctx, big, small):
    """larger -> smaller -> larger: nothing of the previous parse's compact view (DONE bits) or level arrays (entries beyond
    the new sizes) is read"""
    for name in (big, small, big, small):
        doc, nd = VALID[name]
        check(ctx, doc, nd=nd, what=(big, small, name))


def test_sixteen_tokens_per_lane():
    """SJHIP_S2_ITEMS=16: the tile matcher is compiled for both emit shapes and both leave live brackets to k_br_match.
    The variable is read once per process: the documents run in an interpreter of their own."""
    code = r"""
import sys
sys.path.insert(0, 'simdjson-go_amd'); sys.path.insert(0, 'tests')
import numpy as np
import sjhip, oracle_lib as O, s2_brackets as B
ctx = sjhip.Context(0)
for name, (d, nd) in sorted(B.valid_docs().items()):
    for copy in (True, False):
        ref = O.parse(d, ndjson=nd, copy_strings=copy)
        pj = ctx.parse(d, ndjson=nd, copy_strings=copy)
        assert ref.rc == 0 and np.array_equal(pj.Tape, ref.tape) and np.array_equal(pj.Strings, ref.strings), (name, copy)
for name, d in sorted(B.error_docs().items()):
    want = O.parse(d).rc
    try:
        ctx.parse(d)
        got = 0
    except sjhip.ParseError as e:
        got = e.code
    assert got == want != 0, (name, got, want)
print('ok')
"""
    env = dict(os.environ, SJHIP_S2_ITEMS="16")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-500:], r.stderr[-1500:])


def test_level_4_document(ctx):
    """17 million brackets (25 MB): the five-level tree, k_min_upper building two levels, answers found at level 4 and
    descended from there.  One copy mode."""
    t0 = time.time()
    doc = B.level4_doc()
    ref = O.parse(doc)
    assert ref.rc == 0
    rc, pj = gpu_parse(ctx, doc, False, True)
    assert rc == 0
    assert len(pj.Tape) == len(ref.tape)
    if not np.array_equal(pj.Tape, ref.tape):
        d = np.nonzero(pj.Tape != ref.tape)[0]
        raise AssertionError(("tape differs at", len(d), d[:5], [hex(int(x)) for x in pj.Tape[d[:3]]], [hex(int(x)) for x in ref.tape[d[:3]]]))
    assert np.array_equal(pj.Strings, ref.strings)
    print("level-4 document: %d bytes, %d tape words, %.1f s with the oracle" % (len(doc), len(ref.tape), time.time() - t0))
