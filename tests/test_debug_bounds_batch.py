"""k_batch_pack on the bounds-checked build (libsjhip_dbg.so, csrc/sj_bounds.h): the caller's buffer (up to the end of its last
document), the descriptors and the packed message are checked views there, every 16-byte access and every end check states its
range, and a violation fails the batch call.  The chunk, block, alignment, newline and end-check cases of
tests/test_gpu_batch_seams.py and one staging pair, in their own interpreter with SJHIP_LIB pointing at that build: the oracle's
results and no recorded violation.  The device buffers there end with their last document, so a 16-byte load that runs on past a
document's end, which changes no tape, is a violation here."""
import pytest

import test_gpu_batch_seams as T


@pytest.mark.gpu
def test_batch_seams_run_clean_on_the_debug_build():
    import __graft_entry__ as G
    T.run_on_debug_build(G.build_lib(debug_bounds=True))
