"""The kernel of csrc/sampled_experts.hip compiles for gfx950 without scratch or spills, with the registers DESIGN.md 6.8 quotes."""
from vorta_amd.build import kernel_resources


def test_gather_sample_rows_kernel_has_no_scratch_and_no_spills():
    res = kernel_resources("sampled_experts.hip")
    assert len(res) == 1 and "gather_sample_rows_kernel" in next(iter(res)), list(res)  # one kernel: the rows are moved as bytes
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["lds"] == 0 and r["vgpr"] <= 48, (name, r)  # six 16-byte rows in flight: 8 waves a SIMD
