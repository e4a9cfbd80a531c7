"""The column and list kernels on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h) at their cuts: the cases of
tests/col_geometry.py marked `debug` -- the word / element disagreement, a first failing element at every step and lane with the
shifted words behind it, two failures in a step, and the partial wave (strings, numbers, string lists, and a selection) -- run as
tests/test_gpu_column_seams.py runs them, in their own interpreter with SJHIP_LIB pointing at that build (as
tests/test_debug_bounds_lists.py does).  sjhip_fetch_path_strings ends without the bounds check, so every string-column fetch is
followed by a checked query call on the same context: a violation of k_q_col_gather fails here, not in a later test.
Measured once on an MI355X: the child -- interpreter start, imports and the 21 cases -- took 1.8 s (1.4 s of them inside the
script; profiles/r32_column_seams_time.txt); its limit is ten times that."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")
TIME_S = 1.8  # the child on an MI355X, measured


@pytest.mark.gpu
def test_column_seams_run_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys, time
t0 = time.time()
sys.path[:0] = [%r, %r]
import sjhip
import col_geometry as G
import test_gpu_column_seams as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
cases = [c for c in G.all_cases() if c.debug]
assert {c.family for c in cases} == set(G.MODES) and len(cases) >= 20
for c in cases:
    T.run_case(ctx, c, **({"checked": True} if c.family == "strings" else {}))
print('child seconds %%.1f' %% (time.time() - t0))
print('ok')
""" % (PKG, HERE)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=10 * TIME_S)
    print(out.stdout[-200:].decode())
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
