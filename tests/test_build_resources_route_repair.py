"""The kernel of csrc/route_repair.hip compiles for gfx950 without scratch or spills, with the LDS DESIGN.md 6.8 quotes."""
from vorta_amd.build import kernel_resources


def test_route_repair_kernel_has_no_scratch_and_no_spills():
    res = kernel_resources("route_repair.hip")
    assert len(res) == 1 and "route_repair_kernel" in next(iter(res)), list(res)  # one kernel, one workgroup
    for name, r in res.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        # one table of 1024 four-byte entries (a head's tier * 3 + expert after the rule, and the repaired flag): 4 KiB of the 160 KiB
        assert r["lds"] == 1024 * 4, (name, r)
        assert r["vgpr"] <= 64, (name, r)  # as its siblings: one workgroup of four waves, occupancy is no concern
