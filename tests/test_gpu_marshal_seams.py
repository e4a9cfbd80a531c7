"""GPU: sjhip_marshal_json (k_ms_tile, k_ms_keys and the launches around them, csrc/marshal.hip) with an entry exactly on every
cut of its work -- tile and thread edges, the anchor search's reach, the LDS window of every variant, the 8-byte slots of the
text accumulator, the four queues, the Strings.B stage, the look-back's steps, the key tiles.  The documents are those of
tests/ms_geometry.py; tests/test_ms_geometry.py shows on the CPU that they lie on the cuts they claim and that the builder's
text is the oracle's.

Every document runs in four modes (copying and not, key flags recovered from the tokens and left by the parser); Tape and
Strings.B must be the oracle's and the text the builder's and the oracle's.  A mismatch names the first differing byte and the
tile, tape word and entry that own it."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import ms_geometry as M
import oracle_lib as O
from test_gpu_parse import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_DOCS = {}


def docs(f):
    if f not in _DOCS:
        _DOCS[f] = list(M.family(f))
    return _DOCS[f]


def mismatch(d, got, mode):
    want = d.text
    k = next(i for i in range(min(len(got), len(want)) + 1) if got[i:i + 1] != want[i:i + 1])
    tile, word, kind, j = M.owner(d, min(k, len(want) - 1))
    return AssertionError((d.name, mode, "lengths", len(got), len(want), "first difference at byte", k, "got", got[max(0, k - 30):k + 30],
                           "want", want[max(0, k - 30):k + 30], "owned by tile", tile, "tape word", word, "word in tile", word % M.TILE,
                           "entry", kind, d.pieces[j][:40]))


def check_marshal(ctx, d):
    for copy in (True, False):
        ref = O.parse(d.data, ndjson=d.nd, copy_strings=copy)
        assert ref.rc == 0, d.name
        rc, want = O.marshal_json(ref.tape, ref.strings, d.data[ref.msg_off:ref.msg_off + ref.msg_len])
        assert rc == 0 and want == d.text, d.name
        for kf in (False, True):
            pj = ctx.parse(d.data, ndjson=d.nd, copy_strings=copy, key_flags=kf)
            assert np.array_equal(pj.Tape, ref.tape) and pj.Strings.tobytes() == ref.strings.tobytes(), (d.name, copy, kf)
            got = ctx.marshal_json()
            if got != d.text:
                raise mismatch(d, got, (copy, kf))


@pytest.mark.parametrize("f", ["a", "b", "f", "h"])
def test_family(ctx, f):
    for d in docs(f):
        check_marshal(ctx, d)


@pytest.mark.parametrize("window", M.WINDOWS + ("short entries",))
def test_window_edges(ctx, window):
    mine = [d for d in docs("c") if d.info.get("window", "short entries") == window]
    assert len(mine) == (2 if window == "short entries" else 3)
    for d in mine:
        check_marshal(ctx, d)


@pytest.mark.parametrize("part", ["clean", "one", "three", "other", "long fitting", "long over"])
def test_slot_alignment(ctx, part):
    mine = [d for d in docs("d") if (d.info["part"] + {True: " fitting", False: " over"}.get(d.info.get("fits"), "")) == part]
    assert len(mine) == 1
    check_marshal(ctx, mine[0])


QUEUES = ("1024 x", "short/long", "int/float", "short strings", "long strings", "object")


@pytest.mark.parametrize("queue", QUEUES)
def test_queues(ctx, queue):
    mine = [d for d in docs("e") if queue in d.name]
    assert mine and all(sum(q in d.name for q in QUEUES) == 1 for d in docs("e"))  # (no document is left out)
    for d in mine:
        check_marshal(ctx, d)


@pytest.mark.parametrize("tiles", M.G_TILES)
def test_tile_counts(ctx, tiles):
    mine = [d for d in docs("g") if d.info["tiles"] == tiles]
    assert len(mine) == (3 if tiles in (65, 129) else 1)
    for d in mine:
        check_marshal(ctx, d)


def test_large_small_large_on_one_context(ctx):
    """a stale descriptor, ticket, slen or cnt_s of the call before would show"""
    g = {d.info["tiles"]: d for d in docs("g") if d.info["form"] == "plain"}
    small = [d for d in docs("a") if M.n_words(d) < 10]
    assert len(small) >= 6
    for d in (g[130], small[0], g[129], small[1], g[1], g[66], small[-1], g[65]):
        check_marshal(ctx, d)


@pytest.mark.parametrize("which", ["floats", "integers"])
def test_number_sweep(ctx, which):
    d, = [d for d in docs("i") if d.name == "i " + which]
    check_marshal(ctx, d)


# ---- the variables that are read once per process -----------------------------------------------------------------------------------
CHILD = r"""
import pickle, sys
sys.path[:0] = [%r, %r]
import sjhip
if %r:
    assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
docs = pickle.load(open(sys.argv[1], 'rb'))
modes = [(c, k) for c in (True, False) for k in (False, True)]
ctx = sjhip.Context(0)
for i, (name, data, nd, text) in enumerate(docs):
    for copy, kf in modes:
        ctx.parse(data, ndjson=nd, copy_strings=copy, key_flags=kf)
        got = ctx.marshal_json()
        if got != text:
            print('MISMATCH %%d %%d %%d' %% (i, copy, kf))
            sys.stdout.flush()
            open(sys.argv[1] + '.got', 'wb').write(got)
            sys.exit(3)
print('ok %%d' %% len(docs))
"""


def run_child(tmp_path, ds, env, debug_lib=None, timeout=300):
    """the documents in a fresh interpreter with `env` (no exec: a child process), compared with the builder's text there"""
    path = str(tmp_path / "docs.pickle")
    with open(path, "wb") as f:
        pickle.dump([(d.name, d.data, d.nd, d.text) for d in ds], f)
    if debug_lib:
        env = dict(env, SJHIP_LIB=debug_lib)
    code = CHILD % (os.path.join(ROOT, "simdjson-go_amd"), HERE, bool(debug_lib))
    r = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=timeout)
    out = r.stdout.strip().splitlines()
    if r.returncode == 3 and out and out[-1].startswith("MISMATCH"):
        i, copy, kf = map(int, out[-1].split()[1:])
        raise mismatch(ds[i], open(path + ".got", "rb").read(), (env, bool(copy), bool(kf)))
    assert r.returncode == 0 and out and out[-1] == "ok %d" % len(ds), (env, r.returncode, r.stdout[-500:], r.stderr[-1500:])


ENVS = [{}, {"SJHIP_MS_VARIANT": "0"}, {"SJHIP_MS_VARIANT": "3"}, {"SJHIP_MS_VARIANT": "5"}, {"SJHIP_MS_VARIANT": "6"},
        {"SJHIP_MS_VARIANT": "7"}, {"SJHIP_MS_ONEPASS": "0"}, {"SJHIP_MS_ONEPASS": "0", "SJHIP_MS_VARIANT": "7"},
        {"SJHIP_MS_TEST_BOUND": "4096"}]


@pytest.mark.parametrize("env", ENVS, ids=lambda e: ",".join("%s=%s" % (k[9:], v) for k, v in e.items()) or "default")
def test_families_under_every_variant(tmp_path, env):
    """families a - h (no number sweep) with every shape of the tile kernel, with the single pass turned off, and with a text bound of
    4 KiB, under which every document of more than one tile falls back to the two-pass form"""
    run_child(tmp_path, [d for f in "abcdefgh" for d in docs(f)], env)


@pytest.mark.parametrize("short_by", [0, 1])
def test_bound_at_the_text_length(tmp_path, short_by):
    """The 65-tile document with the single pass's text bound at exactly its text length (the last tile ends on the bound) and one
    byte below it (the last tile reports that the bound did not hold, the two-pass form runs).  Which of the two ran cannot be
    seen from outside: both must give the same text."""
    d, = [d for d in docs("g") if d.info["tiles"] == 65 and d.info["form"] == "plain"]
    run_child(tmp_path, [d], {"SJHIP_MS_TEST_BOUND": str(len(d.text) - short_by)})
