"""sjhip_marshal_rows_paths on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the per-cell index, the per-row lengths,
the name pieces and their offsets are reached through checked views (A_MPROJ_IDX, A_MPROJ_OFF, A_MPROJ_NAMES, A_MPROJ_NAME_OFF), the
text and the row offsets through A_MROWS_TEXT / A_MROWS_OUT_OFF, the source through A_TAPE / A_ROWS / A_KEYFLAG and ms_string, and a
violation fails the call.  The row-count, cell-size, string, name and absence documents of tests/test_gpu_marshal_rows_paths.py, once,
in their own interpreter with SJHIP_LIB pointing at that build (as tests/test_debug_bounds_marshal_rows.py runs the whole rows)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_marshal_rows_paths_runs_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_marshal_rows_paths as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
for n in (0, 1, 5, 257, 1025):
    T.check_row_count(ctx, n)
T.test_one_column_sixteen_columns_and_the_limits_of_a_plan(ctx)
T.check_cell_sizes(ctx)
for copy in (True, False):
    for kf in (True, False):
        T.check_strings(ctx, copy, kf)
        T.check_parse_mode(ctx, copy, kf)
T.check_names(ctx)
T.check_absence(ctx)
T.test_row_kinds_prefix_paths_and_one_path_twice(ctx)
T.test_composition_with_the_selecting_calls(ctx)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
