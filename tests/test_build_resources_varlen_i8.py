"""The kernels of csrc/attn_fwd_i8_varlen.hip compile for gfx950 without scratch or vector spills, with the LDS DESIGN.md 6.12
quotes (the int8-score family's 70 656 B: at most 80 KiB, so two workgroups fit a CU)."""
from vorta_amd.build import kernel_resources


def test_int8_varlen_kernels_have_no_scratch_and_no_vector_spills():
    res = kernel_resources("attn_fwd_i8_varlen.hip")
    assert len(res) == 4, list(res)  # bf16 / fp16 x 128 / 256 rows
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["lds"] == 70656 <= 80 * 1024, (name, r)
