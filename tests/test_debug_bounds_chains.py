"""Call chains on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): eight chains of tests/test_gpu_chains.py
(chain_model.DEBUG_CHAINS: fresh contexts among them, and chains that unnest twice) in an interpreter of their own with SJHIP_LIB
pointing at that build, as tests/test_debug_bounds_where_multi.py does -- a stale or short view of a work array or an arena then
fails the call instead of reading a neighbour's bytes.  The same for chain_model.DEBUG_CHAINS_M, eight chains of the extended generator."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "simdjson-go_amd")


def run_child(code, lib):
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    print(out.stdout.decode()[-300:])
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-3000:], out.stderr[-3000:])


@pytest.mark.gpu
@pytest.mark.parametrize("half", (0, 1))
def test_member_chains_run_clean_on_the_debug_build(half):
    """chain_model.DEBUG_CHAINS_M, eight chains of the extended generator (member rows twice, parent counts one past a multiple
    of 32 in front of unnest_members, fresh contexts), in children of their own, by the route of the case below -- four chains
    a child: the start of an interpreter and the load of the library are most of a case's time"""
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys, time
t0 = time.time()
sys.path[:0] = [%r, %r, %r]
import sjhip
import chain_model as CM
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
shared = sjhip.Context(0)
t1 = time.time()
for k in CM.DEBUG_CHAINS_M[%d::2]:
    chain = CM.CHAINS_M[k]
    ctx = sjhip.Context(0) if chain[3] else shared
    CM.run_on(ctx, chain, extended=True)
    if chain[3]:
        ctx.close()
print('imports, library load and first context: %%.2f s; four chains: %%.2f s' %% (t1 - t0, time.time() - t1))
print('ok')
""" % (PKG, HERE, ROOT, half)
    run_child(code, lib)


@pytest.mark.gpu
def test_chains_run_clean_on_the_debug_build():
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    code = r"""
import sys, time
t0 = time.time()
sys.path[:0] = [%r, %r, %r]
import sjhip
import chain_model as CM
assert sjhip.lib().sjhip_debug_bounds_selftest() == 2
shared = sjhip.Context(0)
t1 = time.time()
for k in CM.DEBUG_CHAINS:
    chain = CM.CHAINS[k]
    ctx = sjhip.Context(0) if chain[3] else shared
    CM.run_on(ctx, chain)
    if chain[3]:
        ctx.close()
print('imports, library load and first context: %%.2f s; the eight chains: %%.2f s' %% (t1 - t0, time.time() - t1))
print('ok')
""" % (PKG, HERE, ROOT)
    env = dict(os.environ, SJHIP_LIB=lib)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    print(out.stdout.decode()[-300:])
    assert out.returncode == 0 and out.stdout.strip().endswith(b"ok"), (out.stdout[-3000:], out.stderr[-3000:])
