"""Row predicates on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the flags, the prefixes, the new row offsets
and the new row index are reached through checked views (A_WHERE_FLAG, A_WHERE_PRE, A_WHERE_OFF, A_ROWS), and a violation fails
the call.  The parity cases of tests/test_gpu_where.py and a tile seam, in their own interpreter with SJHIP_LIB pointing at that
build (as tests/test_debug_bounds_rows.py runs the row selection)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_where_runs_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_where as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
for copy in (True, False):
    T.test_parity_on_items(ctx, copy)
    T.test_parity_on_records(ctx, copy)
T.test_record_counts_at_the_seams(ctx, 1025)
T.test_records_owning_0_to_7_rows(ctx, 1025)
T.test_empty_path_on_scalar_rows(ctx)
T.test_no_rows_kept(ctx)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
