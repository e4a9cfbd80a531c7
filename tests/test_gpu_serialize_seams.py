"""GPU: sjhip_serialize_ex / sjhip_deserialize (k_ser_tile, k_des_tile and the scans around them, csrc/serialize.hip) with an entry
exactly on every cut of their work -- thread, wave and tile edges of the 2048-word walk, the anchor search's reach and the retry
with the global anchors, the slots of the de-duplication table, the packed per-tile counts, the varint widths of the frame, the
ranges of the one-block scan, the 4096-tag tiles of Deserialize.  The documents are those of tests/ser_geometry.py;
tests/test_ser_geometry.py shows on the CPU that they lie on the cuts they claim and that the model's streams are the oracle's.

Every comparison is exact.  A mismatch names the column, the byte, and the tile, thread, tape word and entry that own it."""
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import ser_geometry as S
from test_gpu_parse import ctx  # noqa: F401
from test_ser_geometry import H_ORACLE_READS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@functools.lru_cache(maxsize=None)
def reference(f, i):
    """-> (the oracle's plain stream, the expected de-duplicated stream, {stream: the oracle's Deserialize of it})"""
    d = S.family(f)[i]
    r = O.parse(d.data, ndjson=d.nd, copy_strings=True)
    assert r.rc == 0, d.name
    plain = O.serialize(r.tape, r.strings, bytes(d.data[r.msg_off:r.msg_off + r.msg_len]), dedup=False)[0].tobytes()
    dedup = plain if d.big else d.stream(True)  # (a document built by multiplication holds no string)
    assert d.big or d.stream(False) == plain, d.name
    des = {}
    for s in {plain, dedup}:
        rc, tape, strs, msg = O.deserialize(s)
        assert rc == 0, d.name
        des[s] = (tape, len(strs), bytes(msg))
    return plain, dedup, des


def check(ctx, f, i):
    """-> the failures of document i of family f, one line each"""
    d = S.family(f)[i]
    plain, dedup, des = reference(f, i)
    failed = []
    ctx.parse(d.data, ndjson=d.nd, copy_strings=True)
    for form, want in ((False, plain), (True, dedup)):
        sizes = ctx.serialize(fetch=False, dedup=form)
        got = bytes(ctx.serialize(dedup=form))
        u = S.unframe(want)
        if sizes != {"tags": len(u["tags"]), "values": len(u["values"]), "strings": len(u["strings"]), "stream": len(want)}:
            failed.append((d.name, "sizes", form, sizes))
        if form and not d.big:
            try:
                bad = S.valid_dedup(got, d)
            except (AssertionError, IndexError) as e:
                bad = ["not a stream: %r" % (e,)]
            if bad:
                failed.append((d.name, "valid_dedup (any table policy)", bad[:3]))
        if got != want:
            failed.append(("exact", S.describe(d, got, form) if not d.big else (d.name, form, len(got), len(want))))
    for s, (tape, nstr, msg) in des.items():
        pj = ctx.deserialize(np.frombuffer(s, dtype=np.uint8))
        if not np.array_equal(pj.Tape, tape):
            k = int(np.flatnonzero(pj.Tape[:len(tape)] != tape[:len(pj.Tape)])[0]) if len(pj.Tape) == len(tape) else -1
            failed.append((d.name, "Deserialize: tape", len(pj.Tape), len(tape), "first differing word", k, "tag tile of its tag unknown; tile", k // S.TILE))
        if pj.Message != msg or len(pj.Strings) != nstr or msg != S.unframe(s)["strings"]:
            failed.append((d.name, "Deserialize: Message or Strings"))
    return failed


@pytest.mark.parametrize("order", ["forward", "reverse"])
@pytest.mark.parametrize("f", sorted(S.FAMILIES))
def test_family(ctx, f, order):
    """the documents of a family on one context, in order and in reverse: the arenas grow and shrink, a closing slot no opener
    wrote would hold a word of the larger run before"""
    idx = list(range(len(S.family(f))))
    failed = []
    for i in (idx if order == "forward" else idx[::-1]):
        failed += check(ctx, f, i)
    assert not failed, failed[:6]


# the corrupt streams the device rejects although the oracle reads them, with the reason
DEVICE_ONLY = {
    "TagNop on the last tag of a thread": "TagNop entries (left by in-place deletions) are not read on the device",
    "TagNop on the last tag of a tile": "TagNop entries (left by in-place deletions) are not read on the device",
}


def test_corrupt_streams(ctx):
    import sjhip
    d, good, muts = S.h_streams()
    rc, tape, strs, msg = O.deserialize(good)
    assert rc == 0 and set(DEVICE_ONLY) <= {n for n, _ in muts}
    wrong = []
    for name, s in muts:
        rc2, tape2, strs2, msg2 = O.deserialize(s)
        assert (rc2 == 0) == (name in H_ORACLE_READS), name
        try:
            pj = ctx.deserialize(np.frombuffer(s, dtype=np.uint8))
            if rc2 != 0 or name in DEVICE_ONLY:
                wrong.append((name, "read by the device"))
            elif not np.array_equal(pj.Tape, tape2) or pj.Message != bytes(msg2):
                wrong.append((name, "read differently"))
        except sjhip.ParseError:
            if rc2 == 0 and name not in DEVICE_ONLY:
                wrong.append((name, "rejected by the device, read by the oracle"))
        pj = ctx.deserialize(np.frombuffer(good, dtype=np.uint8))  # the unmutated stream directly after
        if not np.array_equal(pj.Tape, tape) or pj.Message != bytes(msg):
            wrong.append((name, "the well-formed stream after it"))
    assert not wrong, wrong


# ---- another build of the library, in an interpreter of its own --------------------------------------------------------------------------
CHILD = r"""
import pickle, sys
import numpy as np
sys.path[:0] = [%r, %r]
import sjhip
if %r:
    assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
docs = pickle.load(open(sys.argv[1], 'rb'))
ctx = sjhip.Context(0)
for i, (name, data, nd, plain, dedup) in enumerate(docs):
    ctx.parse(data, ndjson=nd, copy_strings=True)
    for form, want in ((0, plain), (1, dedup)):
        got = bytes(ctx.serialize(dedup=bool(form)))
        if got != want:
            print('MISMATCH %%d %%d' %% (i, form))
            sys.stdout.flush()
            open(sys.argv[1] + '.got', 'wb').write(got)
            sys.exit(3)
    for want in (plain, dedup):
        pj = ctx.deserialize(np.frombuffer(want, dtype=np.uint8))
        assert len(pj.Tape) == ctx.parse(data, ndjson=nd, copy_strings=True).Tape.size, name
print('ok %%d' %% len(docs))
"""


def run_child(tmp_path, ds, env, debug_lib=None, timeout=300):
    """the documents in a fresh interpreter with `env` (no exec: a child process), compared with the model's streams there"""
    path = str(tmp_path / "docs.pickle")
    with open(path, "wb") as f:
        pickle.dump([(d.name, d.data, d.nd, d.stream(False), d.stream(True)) for d in ds], f)
    if debug_lib:
        env = dict(env, SJHIP_LIB=debug_lib)
    code = CHILD % (os.path.join(ROOT, "simdjson-go_amd"), HERE, bool(debug_lib))
    r = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=timeout)
    out = r.stdout.strip().splitlines()
    if r.returncode == 3 and out and out[-1].startswith("MISMATCH"):
        i, form = map(int, out[-1].split()[1:])
        raise AssertionError(S.describe(ds[i], open(path + ".got", "rb").read(), bool(form)))
    assert r.returncode == 0 and out and out[-1] == "ok %d" % len(ds), (env, r.returncode, r.stdout[-500:], r.stderr[-1500:])
