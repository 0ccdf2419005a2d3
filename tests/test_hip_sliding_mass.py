"""GPU: the routed path with key tiles chosen by sampled attention mass (`RoutedGeometry(sliding_keys="mass")`):
every head on the sliding-tile expert, the launches as recorded, against float64 attention over the key lists the selection
itself wrote, at the rule and margin tests/test_hip_sliding_content.py holds the content launch to (`unit_ratios` <= 1 of
tests/_attn_fwd_model.py); "window" and "content" bit for bit what a geometry built without the keyword gives; the refusals."""
import pytest
import torch

import _attn_fwd_model as F
import _random_launch as RL
import test_hip_attention_bwd as B
from test_hip_sliding_content import _geom, _per_slot, _routed

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("model", ["hunyuan", "wan"])
@pytest.mark.parametrize("dtype", F.DTYPES, ids=F.dtype_name)
def test_mass_launch_against_float64_over_its_own_lists(model, dtype, golden):
    from vorta_amd import ops
    _, t, te, q, k, v, _, _ = B._mixture_case(model, dtype, golden, H=2)
    geom = _geom(sliding_keys="mass")
    out, launches = torch.full_like(q, RL.SENTINEL), []
    _routed(q, k, v, geom, model, t, te, out=out, record=launches, fp8=False)
    torch.cuda.synchronize()
    kv = launches[0]["kv_rows"]
    assert kv.dim() == 3 and kv.stride(0) > 0 and launches[0]["kv_rows_stride_g"] == kv.stride(1) > 0
    # the lists are the mass statistic's at the call's softmax scale (the default: D^-0.5), not the tile means'
    q_rows = geom.sta_tables(te)[0]
    by = {s: ops.sta_select_tiles(q[0], k[0], geom.latent, geom.tile, geom.window, te, q_rows, scores=s)[0] for s in ("mass", "mean")}
    assert torch.equal(kv, by["mass"]) and not torch.equal(kv, by["mean"])
    kws = [{n: x for n, x in c.items() if n not in ("q", "k", "v", "out")} for c in _per_slot(launches)]
    ref = lambda **o: sum(F.model_out(kw, q[0], k[0], v[0], dtype, **o) for kw in kws)  # noqa: E731  (disjoint rows, fill 0)
    valid = torch.stack([F.row_masks(kw, q[0].shape)[0] for kw in kws]).any(0)
    assert valid[:, :B.S_VID + te].all() and not valid[:, B.S_VID + te:].any()
    c = dict(f64=ref(round16=False), model=ref(), f32=ref(round16=False, work=torch.float32), valid=valid)
    for unit, x in F.unit_ratios(out[0].cpu(), c).items():
        print(f"{model} {F.dtype_name(dtype)} {unit}: e_hip / bound max {float(x.max()):.3f}")
        assert float(x.max()) <= 1.0, (unit, float(x.max()))
    assert not out[0, :, B.S_VID + te:].view(torch.int16).any()  # padded text rows: zero bits


@pytest.mark.parametrize("name", ["window", "content"])
def test_window_and_content_keep_the_bits_of_a_geometry_without_the_keyword(name, golden, monkeypatch):
    from vorta_amd import routed
    _, t, te, q, k, v, _, _ = B._mixture_case("hunyuan", torch.bfloat16, golden, H=2)
    monkeypatch.setattr(routed, "_sliding_keys", name)  # (a geometry without the keyword follows the process-wide switch)
    assert _geom().sliding_keys == name
    assert torch.equal(_routed(q, k, v, _geom(), "hunyuan", t, te), _routed(q, k, v, _geom(sliding_keys=name), "hunyuan", t, te))


def test_measurements_by_sampled_candidates_refuse_mass_lists(golden, monkeypatch):
    from test_hip_patch_sampled_expert_fidelity import _setup
    from vorta.patch import measured_routes
    from vorta_amd import routed
    _, t, te, q, k, v, _, _ = B._mixture_case("wan", torch.bfloat16, golden, H=2)
    for fn, kw in ((routed.sampled_expert_fidelity, {}), (routed.route_by_fidelity, dict(max_rel_error=0.1))):
        with pytest.raises(ValueError, match=f"{fn.__name__}: sliding_keys='mass'.*per-head sampled form"):
            fn(q, k, v, _geom(sliding_keys="mass"), model="wan", **kw)
    monkeypatch.setattr(routed, "_sliding_keys", "mass")
    with pytest.raises(ValueError, match="measured_routes: sliding_keys='mass'.*per-head sampled form"):
        with measured_routes(_setup("wan")[0], max_rel_error=0.1):
            pass
