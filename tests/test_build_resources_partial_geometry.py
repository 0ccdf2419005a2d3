"""The kernels partial geometry adds (csrc/sta_tables.hip, csrc/coreset.hip) compile for gfx950 without scratch or spills, and
the selection kernel the partial coreset entry point shares with vorta_coreset_select keeps its registers."""
from vorta_amd.build import kernel_resources


def _by_name(source):
    return {next(k for k in ("sta_partial_q_rows", "sta_partial_kv_rows", "coreset_rest", "coreset_select", "sta_q_rows",
                             "sta_kv_rows", "seq_row_map") if k in name) + ("/bf16" if "DF16b" in name else ""): r
            for name, r in kernel_resources(source).items()}


def test_added_kernels_have_no_scratch_and_no_spills():
    sta, cs = _by_name("sta_tables.hip"), _by_name("coreset.hip")
    added = {"sta_partial_q_rows": sta["sta_partial_q_rows"], "sta_partial_kv_rows": sta["sta_partial_kv_rows"],
             "coreset_rest": cs["coreset_rest"]}
    for name, r in added.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, (name, r)
        assert r["vgpr"] <= 24, (name, r)  # index arithmetic only
    for name, r in {**sta, **cs}.items():
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    assert cs["coreset_select"]["lds"] == 1024 and cs["coreset_select/bf16"]["lds"] == 1024
