"""The row selection on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the tile passes reach the tape through its
checked view, the compaction writes row_index through a checked view of its own (A_ROWS) and every query on rows reads it through
one; a violation fails the call.  The tile-boundary and the raw-word cases of tests/test_gpu_rows.py, in their own interpreter
with SJHIP_LIB pointing at that build (as tests/test_debug_bounds_tables.py runs the tables)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_rows_run_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_rows as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
for first in (T.TILE - 9, T.TILE - 5, T.TILE - 1, T.TILE, T.TILE + 1):
    doc = T.padded(first, T.SEAM_ITEMS)
    ctx.parse(doc)
    rw = T.check_selection(ctx, T.oracle_walk(doc, False, True), (b'items',))
    assert rw.rows[0] == first
    T.check_queries(ctx, rw, [(b'a',), (b'b', b'c')], keys=[b'a'])
T.check_raw_words(ctx)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
