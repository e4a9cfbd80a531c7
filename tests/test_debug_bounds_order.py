"""The ordering on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the per-row keys and statuses, the active entries and
the boundary bytes of the one ordering pipeline, the keys and rows of
the sort, its histograms, the arrays of the product and the flags, prefixes and offsets of the narrowing are reached through checked
views (A_ORDER_ROW, A_ORDER_ACT, A_ORDER_BND, A_SORT, A_SORT_HIST, A_ORDER_OUT, A_WHERE_FLAG, A_WHERE_PRE, A_WHERE_OFF, A_ROWS), and a violation fails
the call.  The shapes T + 1 and 2 T + 3, the rows of every status and a limit of tests/test_gpu_order.py, in their own interpreter
with SJHIP_LIB pointing at that build (as tests/test_debug_bounds_group.py runs the grouping)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_order_runs_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_order as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
T.test_shapes(ctx, T.T + 1, "two-alternating")
T.test_shapes(ctx, 2 * T.T + 3, "random-64-bit")
T.test_every_status(ctx)
T.test_limits(ctx, T.T + 1)
T.test_equal_keys_across_the_limit(ctx)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
