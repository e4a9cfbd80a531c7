"""sjhip_marshal_rows on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the per-row lengths, the row offsets, the text
and the recovered key flags are reached through checked views (A_MROWS_OFF, A_MROWS_OUT_OFF, A_MROWS_TEXT, A_MROWS_KF), the source
through A_TAPE / A_ROWS / A_KEYFLAG and ms_string, and a violation fails the call.  The parity, seam and string documents of
tests/test_gpu_marshal_rows.py, in their own interpreter with SJHIP_LIB pointing at that build (as
tests/test_debug_bounds_filter_rows.py runs the filtered rows)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_marshal_rows_runs_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_marshal_rows as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
T.test_parity_on_items(ctx)
for n in (0, 1, 5, 65, 257, 1025):
    T.test_row_counts_at_the_seams(ctx, n)
T.check_row_lengths(ctx)
T.check_one_long_row(ctx)
for copy in (True, False):
    for kf in (True, False):
        T.check_strings(ctx, copy, kf)
T.test_recovered_key_flags_on_a_long_tape(ctx)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
