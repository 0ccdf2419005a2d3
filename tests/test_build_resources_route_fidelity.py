"""The kernel of csrc/route_fidelity.hip compiles for gfx950 without scratch or spills, with the LDS DESIGN.md 6.8 quotes."""
from vorta_amd.build import kernel_resources


def test_route_fidelity_kernel_has_no_scratch_and_no_spills():
    res = kernel_resources("route_fidelity.hip")
    assert len(res) == 1 and "route_fidelity_kernel" in next(iter(res)), list(res)  # one kernel, one workgroup, both modes
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        # three tables of 1024 four-byte entries (expert / candidate, its error, the ranking): 12 KiB of the 160 KiB
        assert r["lds"] == 3 * 1024 * 4, (name, r)
        assert r["vgpr"] <= 64, (name, r)  # one workgroup of four waves: occupancy is no concern, a spill would be
