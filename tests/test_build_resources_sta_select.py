"""The kernels of csrc/sta_select.hip compile for gfx950 without scratch or spills, with the LDS DESIGN.md 6.10 quotes."""
from vorta_amd.build import kernel_resources


def test_sta_select_kernels_have_no_scratch_and_no_spills():
    res = kernel_resources("sta_select.hip")
    means = {n: r for n, r in res.items() if "sta_tile_means_kernel" in n}
    select = {n: r for n, r in res.items() if "sta_select_expand_kernel" in n}
    assert len(means) == 2 and len(select) == 1 and len(res) == 3, list(res)  # bf16 / fp16 means, one selection
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    for name, r in means.items():
        # the 16 row lanes' partial sums, [16][128] floats; 64 registers = eight waves a SIMD: the pass lives on loads in flight
        assert r["lds"] == 16 * 128 * 4 and r["vgpr"] <= 64, (name, r)
    for name, r in select.items():
        # a 64-tile chunk of k means in rows of 129 floats, four q means, and per wave 1024 keys and 1024 list entries
        assert r["lds"] == 64 * 129 * 4 + 4 * 128 * 4 + 2 * 4 * 1024 * 4, (name, r)
        assert r["vgpr"] <= 128, (name, r)  # two workgroups a CU by LDS: registers are not the limit
