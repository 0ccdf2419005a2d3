"""The kernels of csrc/sampled_fidelity.hip compile for gfx950 without scratch or spills, with the registers and the LDS
DESIGN.md 6.8 quotes."""
from vorta_amd.build import kernel_resources


def test_sampled_fidelity_kernels_have_no_scratch_and_no_spills():
    res = kernel_resources("sampled_fidelity.hip")
    partial = {name: r for name, r in res.items() if "sampled_fidelity_partial_kernel" in name}
    final = {name: r for name, r in res.items() if "sampled_fidelity_final_kernel" in name}
    assert len(partial) == 4 and len(final) == 1 and len(res) == 5, list(res)  # bf16 / fp16 x with / without row sums
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    for name, r in partial.items():
        with_rows = "Lb1E" in name
        assert r["lds"] == 80, (name, r)  # the four waves' five values
        assert r["vgpr"] <= (56 if with_rows else 41), (name, r)  # two rows of two tensors in flight: 8 waves a SIMD
    for name, r in final.items():
        assert r["lds"] == 0 and r["vgpr"] <= 16, (name, r)
