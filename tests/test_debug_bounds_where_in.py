"""Row predicates by membership in a set on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): k_q_in_build and
k_q_in_mark reach the set's values, bytes, hashes and table, and the tape, the strings, the row index and the flags, through checked
views, the narrowing behind them is sjhip_where_path's, and a violation fails the call.  The cases of tests/test_gpu_where_in.py in
their own interpreter with SJHIP_LIB pointing at that build (as tests/test_debug_bounds_where_multi.py does)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_where_path_in_runs_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_where_in as T
import where_in_walk as IW
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
for kind in (T.I, T.S):
    T.test_set_sizes(ctx, kind)
T.test_65536_int_values_against_4096_rows(ctx)
for name in sorted(IW.families()):
    T.test_constructed_tables(ctx, name)
T.test_constructed_tables_without_copied_strings(ctx)
for copy in (True, False):
    T.test_string_lengths(ctx, copy)
T.test_conversions_and_rows_without_a_key(ctx)
for n in (1, 63, 64, 65, 256, 257, T.QTILE - 1, T.QTILE, T.QTILE + 1):
    T.test_row_counts_at_the_seams(ctx, n)
T.test_behind_select_rows_unnest_and_where_path(ctx)
T.test_without_a_selection_one_is_created_and_no_rows_launch_nothing(ctx)
T.test_other_products_survive(ctx)
T.test_the_three_largest_groups_passed_back(ctx)
T.test_the_count_touches_nothing(ctx)
T.test_argument_errors_touch_nothing(ctx)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
