"""sjhip_serialize_ex on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): every string a tape word names is checked
against Strings.B (ser_string) and a violation fails the call.  The anchor and retry documents and the de-duplication documents of
tests/ser_geometry.py (families b and c: the unaligned 8-byte reads of ser_hash and ser_equal next to the ends of Strings.B), in
their own interpreter with SJHIP_LIB pointing at that build: the same streams and no recorded violation."""
import pytest

import ser_geometry as S
import test_gpu_serialize_seams as T


@pytest.mark.gpu
def test_serialize_seams_run_clean_on_the_debug_build(tmp_path):
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    T.run_child(tmp_path, [d for f in "bc" for d in S.family(f)], {}, debug_lib=lib, timeout=600)
