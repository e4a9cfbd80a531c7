"""Row predicates over several tests on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the mark kernel of
sjhip_where_paths reaches the tape, the strings, the row index and the flags through checked views, the narrowing behind it is
sjhip_where_path's, and a violation fails the call.  The equivalence cases of tests/test_gpu_where_multi.py, the 1025-row seam and
the 16-deep path, in their own interpreter with SJHIP_LIB pointing at that build (as tests/test_debug_bounds_where.py does)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_where_paths_runs_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_where_multi as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
for copy in (True, False):
    T.test_equivalences_on_items(ctx, copy)
    T.test_equivalences_on_records(ctx, copy)
T.test_record_counts_at_the_seams(ctx, 1025)
T.test_records_owning_0_to_7_rows(ctx, 1025)
T.test_the_deepest_path_and_the_widest_trie(ctx)
T.test_empty_path_predicates(ctx)
T.test_no_rows_kept_and_a_selection_without_rows(ctx)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
