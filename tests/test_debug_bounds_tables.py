"""The table kernel on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): k_q_table_walk reaches every tape word
through the checked view of the tape and writes its columns through checked views of the table arena and of the string columns'
work arrays; the gathers write the bytes through a view of their own; a violation fails the call.  The random and the parking
tables, both copy modes, against tests/column_walk.py, in their own interpreter with SJHIP_LIB pointing at that build (as
tests/test_debug_bounds_columns.py runs the single columns)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_tables_run_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import column_walk as CW, fixtures, oracle_lib as O, query_walk as Q, sjhip, table_walk as TW
from test_gpu_columns import RANDOM_PATHS, random_nd
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
S, SC = TW.COL_STRING, TW.COL_STRING_CVT
kinds = (CW.COL_FLOAT, CW.COL_INT, CW.COL_UINT, CW.COL_BOOL, S, SC)
park = [((b'Make',), S), ((b'Color',), S), ((b'Latitude',), SC), ((b'Make',), CW.COL_FLOAT), ((b'Fine',), SC)]
docs = [(fixtures.load('parking-citations') * 3, park), (random_nd(11, 3000), [(p, kinds[j %% 6]) for j, p in enumerate(RANDOM_PATHS)]),
        (random_nd(11, 3000), [(p, kinds[(j + 3) %% 6]) for j, p in enumerate(RANDOM_PATHS)])]
for data, columns in docs:
    for copy in (True, False):
        ref = O.parse(data, ndjson=True, copy_strings=copy)
        w = Q.Walk(ref.tape, ref.strings, data[ref.msg_off:ref.msg_off + ref.msg_len])
        ctx.parse(data, ndjson=True, copy_strings=copy)
        got = ctx.extract_table(columns)
        for (path, kind), col in zip(columns, got):
            want = TW.single(w, path, kind)
            assert col[-1].tolist() == want[-1], (path, kind, copy)
            if kind in (S, SC):
                assert col[0].tolist() == want[0] and col[1] == want[1], (path, kind, copy)
            else:
                bits = np.uint8 if kind == CW.COL_BOOL else np.uint64
                assert np.array_equal(col[0].view(bits), np.array(want[0], dtype=bits)), (path, kind, copy)
print('ok')
""" % (PKG, HERE)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
