"""The column kernels on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): k_q_col_gather reaches the bytes of a
string through the offset and length a tape word holds, and writes the column through a checked view of its own; a violation
fails the call.  A numeric and a StringCvt extraction on fixtures and generated records, both copy modes, in their own
interpreter with SJHIP_LIB pointing at that build (as tests/test_debug_bounds.py runs the other queries)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


@pytest.mark.gpu
def test_columns_run_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import column_walk as CW, fixtures, oracle_lib as O, query_walk as Q, sjhip
from test_gpu_columns import random_nd
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
ctx = sjhip.Context(0)
docs = [(fixtures.load('parking-citations') * 3, True, [(b'Make',), (b'Latitude',)]),
        (fixtures.load('twitter'), False, [(b'search_metadata', b'count'), (b'search_metadata', b'max_id_str')]),
        (random_nd(21, 2000), True, [(b'a',), (b'a', b'b'), (b'b',)])]
for data, nd, paths in docs:
    for copy in (True, False):
        ref = O.parse(data, ndjson=nd, copy_strings=copy)
        w = Q.Walk(ref.tape, ref.strings, data[ref.msg_off:ref.msg_off + ref.msg_len])
        ctx.parse(data, ndjson=nd, copy_strings=copy)
        for path in paths:
            v, st = ctx.extract_path(path, CW.COL_INT)
            wv, ws = CW.column(w, path, CW.COL_INT)
            assert np.array_equal(st, np.array(ws, dtype=np.uint8)) and np.array_equal(v.view(np.uint64), np.array(wv, dtype=np.uint64))
            off, col, st = ctx.extract_path_strings(path, cvt=True)
            wo, wd, ws = CW.string_column(w, path, True)
            assert off.tolist() == wo and col == wd and st.tolist() == ws, (path, copy)
print('ok')
""" % (PKG, HERE)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-2000:], out.stderr[-3000:])
