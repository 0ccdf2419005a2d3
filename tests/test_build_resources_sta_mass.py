"""The kernels of csrc/sta_mass.hip compile for gfx950 without scratch or spills, with the LDS and registers DESIGN.md 6.11 quotes."""
from vorta_amd.build import kernel_resources


def test_sta_mass_kernels_have_no_scratch_and_no_spills():
    res = kernel_resources("sta_mass.hip")
    mass = {n: r for n, r in res.items() if "sta_tile_mass_kernel" in n}
    reduce = {n: r for n, r in res.items() if "sta_mass_reduce_kernel" in n}
    assert len(mass) == 2 and len(reduce) == 1 and len(res) == 3, list(res)  # bf16 / fp16 scoring, one reduction
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    for name, r in mass.items():
        # two 16 KiB buffers of 64 key rows; 128 registers = two 8-wave workgroups a CU
        assert r["lds"] == 2 * 64 * 256 and r["vgpr"] <= 128, (name, r)
    for name, r in reduce.items():
        assert r["lds"] == 0 and r["vgpr"] <= 128, (name, r)
