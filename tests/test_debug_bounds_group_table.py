"""The key table of the grouping on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h), where the table of row numbers, the
per-row work arrays and the dictionary's bytes are reached through checked views (A_GROUP_TABLE, A_GROUP_ROW, A_GROUP_LEN, A_GROUP_KEYS) and a
violation fails the call: the families of tests/group_table.py whose chains cross the last slot of a table of 64, 128 and 2048
slots -- a probe step that loses its wrap leaves the table there and nowhere else --, one set of keys with a single 64-bit hash,
and the keys on either side of the 32 bytes at which the dictionary copy changes hands.  In their own interpreter with SJHIP_LIB
pointing at that build and nothing preloaded (as tests/test_debug_bounds_group.py runs the grouping's other tests); every case
must also give the results tests/test_gpu_group_table.py asks for."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_key_table_seams_run_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import group_table as GT
import test_gpu_group_table as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
for name in GT.WRAP_FAMILIES:
    T.run_family(ctx, name, True)
for copy in (True, False):
    T.test_full_collisions(ctx, "collide24", copy)
    T.test_across_waves_and_blocks(ctx, "blocks_chain_str", copy)
    T.test_dictionary_copy_seam(ctx, copy)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
