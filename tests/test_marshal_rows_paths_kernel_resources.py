"""The projection kernels of marshal.hip (sjhip_marshal_rows_paths) exist exactly once, stay off scratch and keep at least four
waves per SIMD -- k_mp_measure and k_mp_write carry the float formatter of sj_ftoa.h as the row kernels next to them do, k_mp_walk
the 32 KiB resume stack of the table walk -- and the row kernels keep their own figures beside them.  Compile-only: hipcc's resource
remarks (tools/kernel_resources.py), on the product and on the bounds-checked build."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as KR  # noqa: E402

PROJECTION_KERNELS = ("k_mp_walk", "k_mp_measure", "k_mp_write")
ROW_KERNELS = ("k_mr_measure", "k_mr_tile_sums", "k_mr_tile_apply", "k_mr_write", "k_mr_keyflags<false>", "k_mr_keyflags<true>")


@pytest.mark.parametrize("flags", [(), ("-DSJ_DEBUG_BOUNDS",)], ids=["product", "bounds-checked"])
def test_projection_kernels_use_no_scratch_and_keep_four_waves(flags):
    rows = {}
    for name, vgprs, scratch, occ, lds in KR.kernels_of("marshal.hip", flags):
        rows.setdefault(name.split("(")[0], []).append((vgprs, scratch, occ, lds))
    for k in PROJECTION_KERNELS + ROW_KERNELS:
        assert len(rows.get(k, ())) == 1, (k, sorted(rows))
        vgprs, scratch, occ, lds = rows[k][0]
        assert scratch == 0, (k, vgprs, scratch, occ)
        assert occ >= 4, (k, vgprs, scratch, occ)
    # the float formatter's registers cost the projection no more than they cost the rows: the same 128-VGPR bound holds
    for k in ("k_mp_measure", "k_mp_write"):
        assert rows[k][0][0] <= 128, (k, rows[k][0])
    assert rows["k_mp_walk"][0][3] == 32 * 1024  # 2 x 16 u32 per lane, in LDS
    for name, figures in rows.items():
        if name.startswith("k_ms_tile<"):
            assert all(scratch == 0 for vgprs, scratch, occ, lds in figures), (name, figures)
