"""The sharded ParseND at its seams on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the emitting kernels add the
tape, Strings.B and message bases behind checked views, and a violation fails the parse.  The MultiContext family of
tests/test_gpu_shard_seams.py for n = 1, 3, 8 and the passing in-library document, in their own interpreter with SJHIP_LIB pointing
at that build (as tests/test_debug_bounds_where_in.py does)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_shard_seams_run_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import torch
torch.cuda.init()
import sjhip
import test_gpu_shard_seams as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
for n in (1, 3, 8):
    T.test_family_through_multicontext(n)
T.test_in_library_documents("ok")
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
