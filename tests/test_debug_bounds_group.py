"""The grouping on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the per-row work arrays, the table of row numbers,
the keys and rows of the sort, its histograms, the group offsets, the arrays of the product and the dictionary's bytes are reached
through checked views (A_GROUP_ROW, A_GROUP_LEN, A_GROUP_TABLE, A_SORT, A_SORT_HIST, A_GROUP_OFF, A_GROUP_OUT, A_GROUP_KEYS), and a
violation fails the call.  The rows of every key status, the 300 cycling keys and the long keys of tests/test_gpu_group.py, in their
own interpreter with SJHIP_LIB pointing at that build (as tests/test_debug_bounds_aggregate.py runs the aggregates)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_groups_run_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_group as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
T.test_every_key_status(ctx)
T.test_more_groups_than_one_digit(ctx)
T.test_key_equality(ctx, "long")
T.test_shapes(ctx, T.T + 1, "two-alternating")
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
