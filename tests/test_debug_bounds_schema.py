"""The row schema on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the members' value indices and parents, the
per-member work arrays, the table of member numbers, the status histogram, the run bounds and the product are reached through
checked views (A_SCHEMA_*), the names through the tape's, Strings.B's and the message's (A_TAPE, A_STRINGS, A_MSG), the sort through
A_SORT, and a violation fails the call.  The check functions of tests/test_gpu_schema.py -- the election's seams, equal hashes,
wrapping chains, the names, the types, the rows, a tile seam, the composition and the fixtures -- in their own interpreter with
SJHIP_LIB pointing at that build (as tests/test_debug_bounds_members.py runs the member rows)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_schema_runs_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import sjhip
import test_gpu_schema as T
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
for n in T.ELECTION_COUNTS:
    for pattern in T.PATTERNS:
        T.check_election_seam(ctx, n, pattern)
T.check_election_rounds(ctx)
T.check_leaders(ctx)
for variant in T.COLLIDING:
    T.check_equal_hashes(ctx, variant)
for cap, members in ((64, 32), (128, 64), (2048, 1000)):
    T.check_table_wrap(ctx, cap, members)
T.check_names(ctx)
T.check_types(ctx)
T.check_rows(ctx)
T.check_0_to_7(ctx)
for key_at in (T.D.TILE - 1, T.D.TILE, T.D.TILE + 1):
    T.check_tile_seam(ctx, key_at)
for copy in (True, False):
    T.check_composition(ctx, copy)
    T.check_fixtures(ctx, copy)
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
