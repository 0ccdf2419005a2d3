"""GPU: the differentiable processors (`differentiable=True`) and `Router.forward_autograd`.

Truth: a torch processor restated here -- projections, norm + RoPE (tests/_norm_rope_restate.py), the attention launches
as recorded from the call under test (tests/_attn_restate.py: the coreset ranking and the sliding tables are constants of
the backward), output projections -- run in float64 and differentiated by torch autograd.  Yardstick: the same restatement
in the call's 16-bit dtype.  Rule (tests/test_hip_attention_bwd.py, "bound 2"): per gradient, the relative Frobenius error
of the processor against float64 is at most 2 x that of torch's 16-bit autograd.  VORTA_PROCESSOR_GRAD_ACCURACY_OUT names a
file that receives the ratios."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from _attn_restate import restate
from _norm_rope_restate import norm_rope, rel_err
from _util import dev

pytestmark = pytest.mark.gpu

LATENT, TILE, WINDOW, GROUP = (8, 6, 8), (2, 3, 4), (3, 3, 3), (2, 3, 2)  # the geometry of tests/test_hip_processors.py
S, H, C, T, TE = 8 * 6 * 8, 6, 64, 16, 11
RATIOS = {}


# ------------------------------------------------------------------------------------------------------------- modules
class _HyAttn(nn.Module):  # tests/test_hip_processors.py _HyFakeAttn, restated
    def __init__(self, dual, dtype, seed):
        super().__init__()
        torch.manual_seed(seed)
        D = 128
        self.heads = H
        self.to_q, self.to_k, self.to_v = (nn.Linear(C, H * D) for _ in range(3))
        self.norm_q, self.norm_k = nn.RMSNorm(D, eps=1e-6), nn.RMSNorm(D, eps=1e-6)
        if dual:
            self.add_q_proj, self.add_k_proj, self.add_v_proj = (nn.Linear(C, H * D) for _ in range(3))
            self.norm_added_q, self.norm_added_k = nn.RMSNorm(D, eps=1e-6), nn.RMSNorm(D, eps=1e-6)
            self.to_out = nn.ModuleList([nn.Linear(H * D, C), nn.Identity()])
            self.to_add_out = nn.Linear(H * D, C)
        else:
            self.add_q_proj = self.add_k_proj = self.add_v_proj = None
            self.norm_added_q = self.norm_added_k = None
            self.to_out = None
            self.to_add_out = None
        for m in self.modules():
            if isinstance(m, nn.RMSNorm):
                nn.init.uniform_(m.weight, 0.5, 1.5)
        self.to(dev()).to(dtype)


class _WanAttn(nn.Module):
    """Wan block attention with RMSNorm across all H*128 channels (the fused norm + RoPE path)"""

    def __init__(self, dtype, seed):
        super().__init__()
        torch.manual_seed(seed)
        D = 128
        self.heads = H
        self.add_k_proj = None
        self.to_q, self.to_k, self.to_v = (nn.Linear(C, H * D) for _ in range(3))
        self.norm_q, self.norm_k = nn.RMSNorm(H * D, eps=1e-6), nn.RMSNorm(H * D, eps=1e-6)
        self.to_out = nn.ModuleList([nn.Linear(H * D, C), nn.Identity()])
        for m in (self.norm_q, self.norm_k):
            nn.init.uniform_(m.weight, 0.5, 1.5)
        self.to(dev()).to(dtype)


# --------------------------------------------------------------------------------------------------------- restatement
def _lin(P, name, x):
    return F.linear(x, P[name + ".weight"], P.get(name + ".bias"))


def _heads(x):  # (N, H*128) -> (H, N, 128)
    return x.view(x.shape[0], H, 128).transpose(0, 1)


def _dense(q, k, v, n_valid=None):
    L = k.shape[1] if n_valid is None else n_valid
    o = torch.softmax(q @ k[:, :L].transpose(1, 2) / math.sqrt(128), dim=-1) @ v[:, :L]
    if n_valid is not None and n_valid < q.shape[1]:  # padded text queries come out zero (hunyuan.py:176)
        o = torch.cat([o[:, :L], torch.zeros_like(o[:, L:])], dim=1)
    return o


def _mixture(q, k, v, score, launches, bufs):
    outs = [torch.zeros(q.shape, dtype=q.dtype, device=q.device) for _ in range(3)]
    for c in launches:
        e = next(i for i, b in enumerate(bufs) if b.data_ptr() == c["out"].data_ptr())
        restate({key: val for key, val in c.items() if key not in ("q", "k", "v", "out")}, q, k, v, outs[e])
    return sum(score[0][:, e, None, None] * outs[e] for e in range(3))


def _hy_restated(attn, P, hidden, enc, score, rope, recorded, dense):
    dual = attn.add_q_proj is not None
    x, e = hidden[0], enc[0]
    if not dual:
        x = torch.cat([x, e], dim=0)
    q, k, v = (_heads(_lin(P, n, x)) for n in ("to_q", "to_k", "to_v"))
    q = norm_rope(q, P["norm_q.weight"], 1e-6, rope[0], rope[1], S)
    k = norm_rope(k, P["norm_k.weight"], 1e-6, rope[0], rope[1], S)
    if dual:
        eq, ek, ev = (_heads(_lin(P, n, e)) for n in ("add_q_proj", "add_k_proj", "add_v_proj"))
        eq, ek = norm_rope(eq, P["norm_added_q.weight"], 1e-6), norm_rope(ek, P["norm_added_k.weight"], 1e-6)
        q, k, v = torch.cat([q, eq], dim=1), torch.cat([k, ek], dim=1), torch.cat([v, ev], dim=1)
    o = _dense(q, k, v, S + TE) if dense else _mixture(q, k, v, score, *recorded)
    o = o.transpose(0, 1).reshape(S + T, H * 128)
    hid, en = o[:S], o[S:]
    if dual:
        hid, en = _lin(P, "to_out.0", hid), _lin(P, "to_add_out", en)
    return hid[None], en[None]


def _wan_restated(attn, P, hidden, enc, score, rope, recorded, dense):
    x = hidden[0]
    e = x if enc is None else enc[0]
    q, k, v = _lin(P, "to_q", x), _lin(P, "to_k", e), _lin(P, "to_v", e)
    cs = (None, None) if rope is None else rope
    q = norm_rope(_heads(q), P["norm_q.weight"], 1e-6, *cs, rope_tokens=0 if rope is None else S, across_heads=True)
    k = norm_rope(_heads(k), P["norm_k.weight"], 1e-6, *cs, rope_tokens=0 if rope is None else S, across_heads=True)
    v = _heads(v)
    o = _dense(q, k, v) if dense else _mixture(q, k, v, score, *recorded)
    return (_lin(P, "to_out.0", o.transpose(0, 1).reshape(x.shape[0], H * 128))[None],)


class _RecordLaunches:
    """the launches and expert buffers of the soft mixture as the call under test launched them"""

    def __enter__(self):
        import vorta_amd.routed as rt
        self.rt, self.stock, self.calls = rt, rt.routed_attention, []

        def spy(*a, **kw):
            if kw.get("record") is not None:
                self.calls.append((kw["record"], [b[0] for b in kw["expert_outs"]]))
            return self.stock(*a, **kw)

        rt.routed_attention = spy
        return self

    def __exit__(self, *exc):
        self.rt.routed_attention = self.stock


WANTED = ("hidden", "enc", "routing_score", "to_q.weight", "to_k.weight", "to_v.weight", "to_out.0.weight", "to_add_out.weight",
          "add_q_proj.weight", "add_k_proj.weight", "add_v_proj.weight", "norm_q.weight", "norm_k.weight",
          "norm_added_q.weight", "norm_added_k.weight")


def _compare(what, attn, restated, call, hidden, enc, score, rope, dense, dtype):
    """forward + backward of sum(out * cot) through `call` (the processor) and through the restatement in float64 / dtype"""
    gen = torch.Generator(device="cpu").manual_seed(17)
    leaves = {"hidden": hidden.clone().requires_grad_(True)}
    if enc is not None:
        leaves["enc"] = enc.clone().requires_grad_(True)
    if score is not None and not dense:
        leaves["routing_score"] = score.clone().requires_grad_(True)
    for p in attn.parameters():
        p.grad = None
    with _RecordLaunches() as rec:
        outs = call(leaves["hidden"], leaves.get("enc"), leaves.get("routing_score"))
    outs = outs if isinstance(outs, tuple) else (outs,)
    cots = [torch.randn(o.shape, generator=gen).to(dtype).to(dev()) for o in outs]
    sum((o * c).sum() for o, c in zip(outs, cots)).backward()
    got = {n: t.grad for n, t in leaves.items()}
    got.update({n: p.grad for n, p in attn.named_parameters()})
    assert dense or len(rec.calls) == 1
    recorded = rec.calls[0] if rec.calls else None

    def reference(dt):
        P = {n: p.detach().to(dt).requires_grad_(True) for n, p in attn.named_parameters()}
        L = {n: t.detach().to(dt).requires_grad_(True) for n, t in leaves.items()}
        o = restated(attn, P, L["hidden"], L.get("enc"), L.get("routing_score"), rope, recorded, dense)
        names = list(L) + list(P)
        g = torch.autograd.grad(sum((a * c.to(dt)).sum() for a, c in zip(o, cots)), [dict(L, **P)[n] for n in names],
                                allow_unused=True)
        return dict(zip(names, g)), o

    ref, o64 = reference(torch.float64)
    t16, _ = reference(dtype)
    for o, r in zip(outs, o64):  # the forward is the function the restatement states
        assert rel_err(o, r) < 1.5e-2, what
    checked = 0
    for name in WANTED:
        if ref.get(name) is None:
            continue
        assert got[name] is not None and got[name].shape == ref[name].shape, f"{what}: no gradient for {name}"
        assert torch.isfinite(got[name].float()).all()
        e_hip, e_t = rel_err(got[name], ref[name]), rel_err(t16[name], ref[name])
        print(f"{what} {name}: e_hip {e_hip:.3e} e_torch {e_t:.3e} ratio {e_hip / max(e_t, 1e-300):.3f}")
        RATIOS.setdefault(name, []).append(e_hip / max(e_t, 1e-300))
        assert e_hip <= 2.0 * e_t, f"{what} {name}: e_hip {e_hip:.3e} > 2 x e_torch {e_t:.3e}"
        checked += 1
    return checked


def _hy_case(dtype, seed):
    from vorta_amd.attention import create_sliding_tile_attn_mask_func, get_group_info
    torch.manual_seed(seed)
    hidden = torch.randn((1, S, C), device=dev()).to(dtype)
    enc = torch.randn((1, T, C), device=dev()).to(dtype)
    ang = torch.rand((S, 64), device=dev()) * 6.28
    rope = (ang.cos().repeat_interleave(2, dim=1).contiguous(), ang.sin().repeat_interleave(2, dim=1).contiguous())
    mask = torch.zeros((1, 1, 1, S + T), dtype=torch.bool, device=dev())
    mask[..., :S + TE] = True  # padded text: text_valid < T
    score = torch.softmax(torch.randn((1, H, 3), device=dev()), dim=-1).to(dtype)
    kw = dict(lowres_group_info=get_group_info(LATENT, GROUP, 0.5, dev()), window_size=WINDOW, tile_size=TILE,
              latent_shape=LATENT, flex_attn_mask_func=create_sliding_tile_attn_mask_func(LATENT, WINDOW, TILE, T, TE, dev()))
    return hidden, enc, rope, mask, score, kw


def _wan_case(dtype, seed):
    from vorta_amd.patch import prepare_wan_self_attn_kwargs
    torch.manual_seed(seed)
    hidden = torch.randn((1, S, C), device=dev()).to(dtype)
    enc = torch.randn((1, 40, C), device=dev()).to(dtype)
    ang = torch.rand((S, 64), device=dev(), dtype=torch.float64) * 6.28
    freqs = torch.polar(torch.ones_like(ang), ang)[None, None]  # (1,1,S,D/2) complex, as modeling_wan.py hands it over
    rope = (ang.cos().float().repeat_interleave(2, dim=1).contiguous(), ang.sin().float().repeat_interleave(2, dim=1).contiguous())
    score = torch.softmax(torch.randn((1, H, 3), device=dev()), dim=-1).to(dtype)
    kw = prepare_wan_self_attn_kwargs(dict(latent_shape=LATENT, window_size=WINDOW, tile_size=TILE, lowres_window_size=GROUP,
                                           lowres_reduction_rate=0.5), dev())
    return hidden, enc, freqs, rope, score, kw


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("dual", [True, False], ids=["dual", "single"])
@pytest.mark.parametrize("mode", ["train", "train_original_attn", "dense"])
def test_hunyuan_processor_gradients(mode, dual, dtype):
    from vorta_amd.attention import HunyuanVideoFlashAttnProcessor, HunyuanVideoFlashAttnProcessorTripleTrain
    attn = _HyAttn(dual, dtype, seed=31 + dual)
    hidden, enc, rope, mask, score, kw = _hy_case(dtype, 7)
    cls = HunyuanVideoFlashAttnProcessor if mode == "dense" else HunyuanVideoFlashAttnProcessorTripleTrain
    proc, plain = cls(differentiable=True), cls()
    if mode == "dense":
        call = lambda h, e, sc: proc(attn, h, e, mask, rope)  # noqa: E731
        call0 = lambda p: p(attn, hidden, enc, mask, rope)  # noqa: E731
    else:
        orig = mode == "train_original_attn"
        call = lambda h, e, sc: proc(attn, h, e, mask, rope, use_original_attn=orig, routing_score=sc, **kw)  # noqa: E731
        call0 = lambda p: p(attn, hidden, enc, mask, rope, use_original_attn=orig, routing_score=score, **kw)  # noqa: E731
    with torch.no_grad():  # under no_grad the flag changes nothing: today's path, today's bits
        a, b = call0(proc), call0(plain)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    n = _compare(f"hunyuan {mode} {'dual' if dual else 'single'} {dtype}", attn, _hy_restated, call, hidden, enc, score, rope,
                 mode != "train", dtype)
    assert n >= (7 if mode != "train" else 8) + (7 if dual else 0)
    if mode == "train":  # differentiable=False keeps refusing
        with pytest.raises(NotImplementedError):
            plain(attn, hidden.clone().requires_grad_(True), enc, mask, rope, routing_score=score, **kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("mode", ["train", "train_original_attn", "dense_self", "dense_cross", "train_cross"])
def test_wan_processor_gradients(mode, dtype):
    from vorta_amd.attention import WanAttnProcessor2_0, WanAttnProcessorTripleTrain
    attn = _WanAttn(dtype, seed=41)
    hidden, enc, freqs, rope, score, kw = _wan_case(dtype, 9)
    cls = WanAttnProcessor2_0 if mode.startswith("dense") else WanAttnProcessorTripleTrain
    proc, plain = cls(differentiable=True), cls()
    cross = mode.endswith("cross")
    if cross:  # text cross attention: Sq != Skv, no rotation
        rope, freqs = None, None
    if cls is WanAttnProcessor2_0:
        call = lambda h, e, sc: proc(attn, h, e, None, freqs)  # noqa: E731
        call0 = lambda p: p(attn, hidden, enc if cross else None, None, freqs)  # noqa: E731
    else:
        orig = mode == "train_original_attn"
        call = lambda h, e, sc: proc(attn, h, e, None, freqs, use_original_attn=orig, routing_score=sc, **kw)  # noqa: E731
        call0 = lambda p: p(attn, hidden, enc if cross else None, None, freqs, use_original_attn=orig,  # noqa: E731
                            routing_score=score, **kw)
    with torch.no_grad():
        assert torch.equal(call0(proc), call0(plain))
    n = _compare(f"wan {mode} {dtype}", attn, _wan_restated, call, hidden, enc if cross else None, score, rope, mode != "train",
                 dtype)
    assert n >= (8 if mode == "train" else 7 + cross)
    if mode == "train":
        with pytest.raises(NotImplementedError):
            plain(attn, hidden.clone().requires_grad_(True), None, None, freqs, routing_score=score, **kw)


def test_eval_classes_refuse_and_sequence_parallel_refuses():
    from vorta_amd.attention import (HunyuanVideoFlashAttnProcessorTripleEval, WanAttnProcessor2_0, WanAttnProcessorTripleEval)
    from vorta_amd.ulysses import SP_STATE
    for cls in (HunyuanVideoFlashAttnProcessorTripleEval, WanAttnProcessorTripleEval):
        with pytest.raises(ValueError):
            cls(differentiable=True)
        assert cls(check_input=True).differentiable is False
    attn = _WanAttn(torch.bfloat16, seed=1)
    hidden = torch.randn((1, 64, C), device=dev()).to(torch.bfloat16).requires_grad_(True)
    stock = SP_STATE._enabled
    SP_STATE._enabled = True
    try:
        with pytest.raises(NotImplementedError, match="sequence-parallel"):
            WanAttnProcessor2_0(differentiable=True)(attn, hidden, None, None, None)
    finally:
        SP_STATE._enabled = stock


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_router_forward_autograd(dtype):
    from vorta_amd.patch.router import Router
    torch.manual_seed(3)
    E, heads, B = 256, 24, 2
    r = Router(E, heads).to(dev()).to(dtype)
    with torch.no_grad():
        r.linear.weight.mul_(4.0)  # scores away from 1/3
    temb = torch.randn((B, E), device=dev()).to(dtype)
    with torch.no_grad():
        a, b = r(temb), r.forward_autograd(temb)
    assert a.shape == b.shape == (B, heads, 3) and a.dtype == b.dtype == dtype
    # one 16-bit ulp of a softmax output: the spacing of the format below 1 (scores lie in (0,1))
    ulp = torch.finfo(dtype).eps / 2
    assert (a.float() - b.float()).abs().max().item() <= ulp
    cot = torch.randn((B, heads, 3), device=dev()).to(dtype)
    (r.forward_autograd(temb) * cot).sum().backward()

    def reference(dt):
        w, bias = (p.detach().to(dt).requires_grad_(True) for p in (r.linear.weight, r.linear.bias))
        sc = torch.softmax(F.linear(F.silu(temb.to(dt)), w, bias).view(B, heads, 3), dim=-1)
        return torch.autograd.grad((sc * cot.to(dt)).sum(), [w, bias])

    ref, t16 = reference(torch.float64), reference(dtype)
    for name, got, t, want in zip(("router.weight", "router.bias"), (r.linear.weight.grad, r.linear.bias.grad), t16, ref):
        e_hip, e_t = rel_err(got, want), rel_err(t, want)
        print(f"router {dtype} {name}: e {e_hip:.3e} e_torch {e_t:.3e} ratio {e_hip / max(e_t, 1e-300):.3f}")
        RATIOS.setdefault(name, []).append(e_hip / max(e_t, 1e-300))
        assert e_hip <= 2.0 * e_t


def test_accuracy_summary_written():
    """max / median of e_hip / e_torch per gradient over this module's cases (runs after them)"""
    if not RATIOS:
        return
    lines = [f"processors {name}: cases {len(r)} max {max(r):.3g} median {float(np.median(r)):.3g}"
             for name, r in sorted(RATIOS.items())]
    print("\n".join(lines))
    path = os.environ.get("VORTA_PROCESSOR_GRAD_ACCURACY_OUT")
    if path:
        with open(path, "w") as f:
            f.write("e_hip / e_torch over the cases of tests/test_hip_processors_grad.py (bound: 2)\n" + "\n".join(lines) + "\n")
    assert all(max(r) <= 2.0 for r in RATIOS.values())
