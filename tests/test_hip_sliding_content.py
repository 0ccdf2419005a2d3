"""GPU: the routed path with content-chosen key tiles (`RoutedGeometry(sliding_keys="content")`): every head on
the sliding-tile expert, the launches as recorded, against float64 attention over the key lists the selection kernel itself
wrote -- the rule tests/_attn_fwd_model.py holds the table-driven sliding launch to (`unit_ratios` <= 1) --, the 8-bit
precisions against the native one at the gates of tests/test_hip_i8.py / tests/test_hip_mx.py, the deterministic backward
against float64 autograd through the same lists at the bound of tests/test_hip_attention_bwd.py, "window" bit for bit what a
geometry without the keyword gives, and the refusals.  Geometry of the backward tests: 16 tiles of 24 rows, 12 key tiles."""
import pytest
import torch

import _attn_fwd_model as F
import _random_launch as RL
import test_hip_attention_bwd as B
from test_hip_i8 import I8_REL_GATE
from test_hip_mx import MX_REL_GATE
from _util import dev

pytestmark = pytest.mark.gpu


def _geom(**kw):
    from vorta_amd.routed import RoutedGeometry
    return RoutedGeometry(B.LATENT, B.TILE, B.WINDOW, B.GROUP, 0.5, dev(), **kw)


def _routed(q, k, v, geom, model, t, te, **kw):
    from vorta_amd.routed import HeadRouting, routed_attention
    return routed_attention(q, k, v, HeadRouting.from_expert_ids([2] * q.shape[1], dev()), geom, model=model, text_len=t,
                            text_valid=te, **kw)


def _per_slot(launches):
    """the recorded launches, a (slots, groups, n_kv) key table as one launch per head slot over its plain (groups, n_kv)
    table: the form the restatements of tests/_attn_restate.py walk"""
    out = []
    for c in launches:
        kv = c.get("kv_rows")
        if kv is None or kv.dim() != 3:
            out.append(c)
            continue
        out += [dict(c, kv_rows=kv[y].contiguous(), kv_rows_stride_g=kv.shape[2], head_list=c["head_list"][y:y + 1], n_heads=1)
                for y in range(c["n_heads"])]
    return out


@pytest.mark.parametrize("model", ["hunyuan", "wan"])
@pytest.mark.parametrize("dtype", F.DTYPES, ids=F.dtype_name)
def test_content_launch_against_float64_over_its_own_lists(model, dtype, golden):
    _, t, te, q, k, v, _, _ = B._mixture_case(model, dtype, golden, H=2)
    assert model == "wan" or t > te > 0
    out, launches = torch.full_like(q, RL.SENTINEL), []
    _routed(q, k, v, _geom(sliding_keys="content"), model, t, te, out=out, record=launches, fp8=False)
    torch.cuda.synchronize()
    kv = launches[0]["kv_rows"]  # two slots with lists of their own: both key strides of the launch are non-zero
    assert kv.dim() == 3 and kv.stride(0) > 0 and launches[0]["kv_rows_stride_g"] == kv.stride(1) > 0
    assert not torch.equal(kv[0], kv[1]), "two heads of random data chose the same tiles everywhere"
    kws = [{n: x for n, x in c.items() if n not in ("q", "k", "v", "out")} for c in _per_slot(launches)]
    ref = lambda **o: sum(F.model_out(kw, q[0], k[0], v[0], dtype, **o) for kw in kws)  # noqa: E731  (disjoint rows, fill 0)
    valid = torch.stack([F.row_masks(kw, q[0].shape)[0] for kw in kws]).any(0)
    assert valid[:, :B.S_VID + te].all() and not valid[:, B.S_VID + te:].any()
    c = dict(f64=ref(round16=False), model=ref(), f32=ref(round16=False, work=torch.float32), valid=valid)
    for unit, x in F.unit_ratios(out[0].cpu(), c).items():
        print(f"{model} {F.dtype_name(dtype)} {unit}: e_hip / bound max {float(x.max()):.3f}")
        assert float(x.max()) <= 1.0, (unit, float(x.max()))
    assert not out[0, :, B.S_VID + te:].view(torch.int16).any()  # padded text rows: zero bits


@pytest.mark.parametrize("precision,gate", [("i8pv", I8_REL_GATE), ("fp8pv", MX_REL_GATE)])
def test_8bit_precisions_over_content_lists(precision, gate, golden):
    _, t, te, q, k, v, _, _ = B._mixture_case("hunyuan", torch.bfloat16, golden, H=2)
    geom = _geom(sliding_keys="content")
    native = _routed(q, k, v, geom, "hunyuan", t, te, fp8=False)[0, :, :B.S_VID + te].float()
    got = _routed(q, k, v, geom, "hunyuan", t, te, fp8=precision)[0, :, :B.S_VID + te].float()
    rel = (got - native).flatten(1).norm(dim=1) / native.flatten(1).norm(dim=1)
    print(f"{precision} over content lists, rel. Frobenius per head against native: {rel.tolist()}")
    assert float(rel.max()) <= gate


def test_deterministic_backward_through_content_lists(golden):
    from vorta_amd.routed import HeadRouting, routed_attention, soft_mixture_attention_autograd
    model, dtype = "hunyuan", torch.bfloat16
    _, t, te, q, k, v, sc, G = B._mixture_case(model, dtype, golden)
    geom, kwm = _geom(sliding_keys="content"), dict(model=model, text_len=t, text_valid=te)
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v, sc)]
    out = soft_mixture_attention_autograd(*leaves, geom, backward="deterministic", **kwm)
    (out * G).sum().backward()
    bufs, launches = [torch.empty_like(q) for _ in range(3)], []
    routed_attention(q, k, v, HeadRouting.every_head_everywhere(q.shape[1], dev()), geom, expert_outs=bufs, fp8=False,
                     record=launches, **kwm)
    assert any(c["kv_rows"] is not None and c["kv_rows"].dim() == 3 for c in launches if c["tag"] == "sliding")
    bufs3 = [b[0] for b in bufs]
    ref, _ = B._mixture_reference(_per_slot(launches), bufs3, q, k, v, sc, G, torch.float64)
    y16, _ = B._mixture_reference(_per_slot(launches), bufs3, q, k, v, sc, G, dtype)
    for name, leaf, a, b in zip(("dq", "dk", "dv"), leaves, y16, ref):
        B._bound(name, leaf.grad[0], a, b, "content lists, deterministic")


def test_window_keeps_the_bits_of_a_geometry_without_the_keyword(golden):
    _, t, te, q, k, v, _, _ = B._mixture_case("hunyuan", torch.bfloat16, golden, H=2)
    assert torch.equal(_routed(q, k, v, _geom(), "hunyuan", t, te), _routed(q, k, v, _geom(sliding_keys="window"), "hunyuan", t, te))


def test_measurements_by_sampled_candidates_refuse_content_lists(golden, monkeypatch):
    from test_hip_patch_sampled_expert_fidelity import _setup
    from vorta.patch import measured_routes
    from vorta_amd import routed
    _, t, te, q, k, v, _, _ = B._mixture_case("wan", torch.bfloat16, golden, H=2)
    for fn, kw in ((routed.sampled_expert_fidelity, {}), (routed.route_by_fidelity, dict(max_rel_error=0.1))):
        with pytest.raises(ValueError, match=f"{fn.__name__}: sliding_keys='content'.*per-head sampled form"):
            fn(q, k, v, _geom(sliding_keys="content"), model="wan", **kw)
    monkeypatch.setattr(routed, "_sliding_keys", "content")
    with pytest.raises(ValueError, match="measured_routes: sliding_keys='content'.*per-head sampled form"):
        with measured_routes(_setup("wan")[0], max_rel_error=0.1):
            pass
