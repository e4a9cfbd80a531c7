"""The grouping by several keys on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the per-row and per-column work
arrays, the key lengths, the table, the buffers of the sort, the group offsets and the arrays of the product are reached through
checked views (A_GROUP_ROW, A_GROUP_LEN, A_GROUP_TABLE, A_SORT, A_SORT_HIST, A_GROUP_OFF, A_GROUP_OUT, A_GROUP_KEYS, A_AGG_*), and a
violation fails the call.  The tuple-equality, status and collision cases of tests/test_gpu_group_multi.py, in their own
interpreter with SJHIP_LIB pointing at that build (as tests/test_debug_bounds_order_multi.py runs the order by several keys)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_group_by_several_keys_runs_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_group_multi as M
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
M.test_shapes(ctx, M.T + 1, "17x17")
M.test_shapes(ctx, 2 * M.T + 3, "all-distinct")
M.test_column_boundaries_swaps_and_kinds(ctx)
M.test_eight_columns_that_differ_in_one(ctx)
M.test_key_lengths_empty_against_no_key_and_escapes(ctx, True)
M.test_key_lengths_empty_against_no_key_and_escapes(ctx, False)
M.test_every_status_on_column_1(ctx)
for name in ("collide", "home40", "capacity_step", "blocks_collide", "blocks_cycle"):
    M.test_table_families(ctx, name)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
