"""CPU-side check of the compiled norm + RoPE backward kernels (hipcc cross-compiles gfx950 without a GPU): no scratch, no
spill, in any instantiation -- the across-heads form holds a whole token of x and g in registers."""
import os

import pytest

from vorta_amd import build

pytestmark = pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="needs hipcc")


def test_norm_rope_bwd_kernels_do_not_spill():
    res = build.kernel_resources("qk_norm_rope_bwd.hip")
    # 2 dtypes x 2 (with / without dweight) x (1 per-head + 3 across-heads) + the final sum
    assert len(res) == 17, sorted(res)
    for name, r in res.items():
        print(name, r)
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 512 and r["lds"] <= 20 * 1024, (name, r)
