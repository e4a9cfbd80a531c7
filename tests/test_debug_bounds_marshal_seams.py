"""sjhip_marshal_json on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): every string a tape word names is checked
against the buffer it points into (ms_string) and a violation fails the call.  The stage and buffer-end documents and the slot
alignment documents of tests/ms_geometry.py (families f and d: the reads next to the ends of Strings.B and of the message), in
their own interpreter with SJHIP_LIB pointing at that build, all four modes: the same text and no recorded violation."""
import pytest

import test_gpu_marshal_seams as T


@pytest.mark.gpu
def test_marshal_seams_run_clean_on_the_debug_build(tmp_path):
    import __graft_entry__ as G
    lib = G.build_lib(debug_bounds=True)
    T.run_child(tmp_path, [d for f in "fd" for d in T.docs(f)], {}, debug_lib=lib, timeout=600)
