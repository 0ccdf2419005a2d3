"""Compiles, no GPU: the code-object figures of route_budget_tiers.hip through `build.kernel_resources`.  The kernel keeps
the rel of every (pair, head) and the routed pairs in LDS (9 x 1024 floats + 1024 ints + the reduction words) and its heads'
two candidate pairs in registers: nothing may go to scratch, and the static LDS must fit the 64 KiB a workgroup may ask for."""


def test_route_budget_tiers_kernel_has_no_scratch_no_spills_and_fits_lds():
    from vorta_amd import build
    assert "route_budget_tiers.hip" in build.SOURCES
    res = build.kernel_resources("route_budget_tiers.hip")
    kernels = {name: r for name, r in res.items() if "route_budget_tiers_kernel" in name}
    assert len(kernels) == 1, res
    (name, r), = kernels.items()
    print(name, r)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert 9 * 1024 * 4 + 1024 * 4 <= r["lds"] <= 64 * 1024, r
    assert r["vgpr"] <= 128, r  # (256 lanes: far from bounding anything; DESIGN.md 6.8 quotes the figure)
