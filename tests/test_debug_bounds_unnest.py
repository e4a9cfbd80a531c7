"""The unnest on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the parents' ranges and statuses, the parent of
every new row, the parent offsets and the new row index are reached through checked views (A_UNNEST_RANGE, A_UNNEST_STATUS,
A_UNNEST_PARENT, A_UNNEST_OFF, A_ROWS), and a violation fails the call.  The fixture cases of tests/test_gpu_unnest.py, the tile
seams and the records owning 0 to 7 parents owning 0 to 7 children, in their own interpreter with SJHIP_LIB pointing at that build
(as tests/test_debug_bounds_where.py runs the row predicates)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_unnest_runs_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_unnest as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
for copy in (True, False):
    T.test_fixtures(ctx, copy)
for first in (T.TILE - 14, T.TILE - 4, T.TILE - 1, T.TILE, T.TILE + 1):
    T.check_tile_seam(ctx, first)
T.check_anchor_retry(ctx)
T.check_0_to_7(ctx)
T.test_no_parents_and_no_rows(ctx)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
