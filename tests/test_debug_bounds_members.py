"""The member rows on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the parents' ranges and statuses, the parent of
every new row, the parent offsets and the new row index are reached through the unnest's checked views (A_UNNEST_RANGE,
A_UNNEST_STATUS, A_UNNEST_PARENT, A_UNNEST_OFF, A_ROWS), the names through the tape's and the column's (A_TAPE, A_COL), the name
predicate through the row predicates' (A_WHERE_*), and a violation fails the call.  The fixture cases of tests/test_gpu_members.py,
the tile seams, the records owning 0 to 7 parents owning 0 to 7 members and the empty cases, in their own interpreter with
SJHIP_LIB pointing at that build (as tests/test_debug_bounds_unnest.py runs the unnest)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_members_run_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_members as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
for copy in (True, False):
    T.check_fixtures(ctx, copy)
for key_at in (T.TILE - 14, T.TILE - 2, T.TILE - 1, T.TILE, T.TILE + 1):
    T.check_tile_seam(ctx, key_at)
T.check_anchor_retry(ctx)
T.check_0_to_7(ctx)
T.check_empty(ctx)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
