"""sjhip_filter_rows on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the per-row work arrays, the new tape and the
new Strings.B are reached through checked views (A_FROWS_WORDS, A_FROWS_STR, A_FROWS_TAPE, A_FROWS_STRINGS), the source through
A_TAPE / A_STRINGS / A_ROWS, and a violation fails the call.  The parity, seam and raw-word cases of tests/test_gpu_filter_rows.py,
in their own interpreter with SJHIP_LIB pointing at that build (as tests/test_debug_bounds_where.py runs the row predicates)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_filter_rows_runs_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_filter_rows as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
T.test_parity_on_items(ctx)
T.test_equals_filter_where_on_parking(ctx)
for n in (0, 1, 5, 65, 257, 1025):
    T.test_row_counts_at_the_seams(ctx, n)
T.check_row_lengths(ctx)
T.check_raw_words(ctx)
T.test_strings_edge_cases(ctx)
T.test_scalar_rows(ctx)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
