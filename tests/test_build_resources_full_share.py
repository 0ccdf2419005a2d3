"""The kernels of csrc/attn_fwd_tilelist.hip and csrc/sta_share_all.hip compile for gfx950 without scratch or vector spills,
with the LDS DESIGN.md 6.13 quotes."""
import pytest

from vorta_amd.build import kernel_resources


@pytest.mark.parametrize("source,kernels,lds", [("attn_fwd_tilelist.hip", 4, 4 * 64 * 256 + 1024 * 4),  # 2 + 2 tiles, the tile list
                                                ("sta_share_all.hip", 2, None)])
def test_new_kernels_have_no_scratch_and_no_vector_spills(source, kernels, lds):
    res = kernel_resources(source)
    assert len(res) == kernels, list(res)
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert lds is None or r["lds"] == lds, (name, r)
