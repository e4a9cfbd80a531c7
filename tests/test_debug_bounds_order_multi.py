"""The order by several keys on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the per-row statuses and keys, the class
keys and the active entries of the rounds, the boundary bytes, the ranked rows and the buffers of both sorts, the arrays of the
product and the flags, prefixes and offsets of the narrowing are reached through checked views (A_ORDER_ROW, A_ORDER_ACT,
A_ORDER_BND, A_SORT, A_SORT_HIST, A_ORDER_OUT, A_WHERE_FLAG, A_WHERE_PRE, A_WHERE_OFF, A_ROWS), and a violation fails
the call.  The shapes T + 1 and 2 T + 3, the mixed kinds, the different-rounds family, every status and one limit of
tests/test_gpu_order_multi.py, in their own interpreter with SJHIP_LIB pointing at that build (as
tests/test_debug_bounds_order_strings.py runs the string order)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_order_by_several_keys_runs_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_order_multi as M
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
M.test_row_counts(ctx, M.T + 1, "pairs")
M.test_row_counts(ctx, 2 * M.T + 3, "three-classes")
M.test_row_counts(ctx, 2 * M.T + 3, "all-equal")
for cols in ([((b"s",), M.S, False), ((b"i",), M.I, False)], [((b"i",), M.I, True), ((b"s",), M.S, True)],
             [((b"f",), M.F, True), ((b"s",), M.S, False), ((b"u",), M.U, True)]):
    M.test_mixed_kinds(ctx, cols)
M.test_string_ties_that_end_in_different_rounds(ctx, True)
M.test_string_ties_that_end_in_different_rounds(ctx, False)
M.test_every_status_on_either_column_and_on_both(ctx)
M.test_limits(ctx, M.T + 1)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
