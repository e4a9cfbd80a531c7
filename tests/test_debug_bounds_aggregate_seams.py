"""The seams of the segmented reduction on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the items every level
hands to the next (A_AGG_ITEMS -- from 32 769 rows on a level reads the items of a level that is itself more than one tile), the
head flags (A_AGG_HEAD) and the per-record results (A_AGG_OUT) are checked views there, and a violation fails the call.  The
fold_seams cases of tests/test_gpu_aggregate_seams.py, one floats case and one group over a fold tile, in their own interpreter
with SJHIP_LIB pointing at that build (as tests/test_debug_bounds_aggregate.py runs the shapes of one level).

The timeout: the child spends its time in the Python walks of sixteen documents of 33 000 to 66 000 rows and one of 98 000 --
13 s measured on an MI355X box (tests/test_debug_bounds_aggregate.py: 0.7 s) --; the limit is ten times that."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_aggregate_seams_run_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import agg_geometry as G
import test_gpu_aggregate_seams as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
for name in T.CASES["fold_seams"]:
    for kind in T.KINDS:
        T.test_fold_seams(ctx, name, kind)
T.test_floats(ctx, G.THREE + ", mixed magnitudes")
T.test_groups_over_a_fold_tile(ctx, "every third row", T.I)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=130)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
