"""The aggregates on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the head flags, the items a level of the
segmented reduction hands to the next, the row offsets and the per-record results are reached through checked views (A_AGG_HEAD,
A_AGG_ITEMS, A_WHERE_OFF, A_AGG_OUT), and a violation fails the call.  The segment shapes, the records without a selection and the rows of every status of
tests/test_gpu_aggregate.py, in their own interpreter with SJHIP_LIB pointing at that build (as tests/test_debug_bounds_where.py
runs the row predicates)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_aggregates_run_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_aggregate as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
for name in ("mixed", "one-record", "one-row-each"):
    T.test_segment_geometry(ctx, name)
T.test_records_without_a_selection(ctx, T.T + 3)
T.test_every_status(ctx)
T.test_empty_path_histogram(ctx)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
