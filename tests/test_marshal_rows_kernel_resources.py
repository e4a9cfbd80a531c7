"""The row kernels of marshal.hip (sjhip_marshal_rows) exist exactly once, stay off scratch and keep at least four waves per SIMD --
k_mr_measure and k_mr_write carry the float formatter of sj_ftoa.h, which once spilled in MarshalJSON -- and k_ms_tile's
instantiations stay off scratch beside them.  Compile-only: hipcc's resource remarks (tools/kernel_resources.py), on the product
and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

ROW_KERNELS = ("k_mr_measure", "k_mr_tile_sums", "k_mr_tile_apply", "k_mr_write", "k_mr_keyflags<false>", "k_mr_keyflags<true>")


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_row_kernels_use_no_scratch_and_keep_four_waves(flags):
    rows = [(name.split("(")[0], vgprs, scratch, occ) for name, vgprs, scratch, occ, lds in KR.kernels_of("marshal.hip", flags)]
    names = [r[0] for r in rows]
    for k in ROW_KERNELS:
        assert names.count(k) == 1, (k, sorted(names))
        name, vgprs, scratch, occ = rows[names.index(k)]
        assert scratch == 0, (k, vgprs, scratch, occ)
        assert occ >= 4, (k, vgprs, scratch, occ)
    tiles = [r for r in rows if r[0].startswith("k_ms_tile<")]
    assert len(tiles) >= 3
    for name, vgprs, scratch, occ in tiles:
        assert scratch == 0, (name, vgprs, scratch, occ)
