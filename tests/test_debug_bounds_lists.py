"""The list-column kernels on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): they reach the elements of an array
through the close index its opening word holds, the bytes of a string through the offset and length of a tape word, and write
values, string offsets and bytes through checked views of their own; a violation fails the call.  A compact version of
tests/test_gpu_lists.py -- generated records, long arrays with their bad elements, both copy modes -- in its own interpreter with
SJHIP_LIB pointing at that build (as tests/test_debug_bounds_columns.py runs the scalar columns)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_lists_run_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import sjhip
import test_gpu_lists as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
ok = ",".join(["7", "2.5"] * 400)
long_lines = ['{"a":[%%s]}' %% ok, '{"a":[%%s,"bad",%%s]}' %% (ok, ok), '{"a":[%%s,1e300,%%s]}' %% (ok, ok), '{"a":[%%s,true,1e300,-1]}' %% ok,
              '{"a":[%%s]}' %% ",".join('"%%s"' %% ("s" * (k %% 150)) for k in range(400)), '{"a":[%%s,null,"x"]}' %% ",".join(['"q"'] * 300)]
doc = T.random_nd(41, 800) + b"\n" + "\n".join(long_lines).encode()
for copy in (True, False):
    T.check_doc(ctx, doc, True, [(b"a",), (b"a", b"b"), (b"b",)], copy)
T.check_doc(ctx, b'{"e":[]}\n{"e":null}', True, [(b"e",), (b"x",)], True)
print('ok')
""" % (PKG, HERE)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
