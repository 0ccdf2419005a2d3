"""A torch restatement of a whole patched mini transformer (tests/_mini_diffusers.py) for tests/test_hip_patch_training.py:
a second instance of the model's class with the model's weights, in any dtype on any device, whose attention processors
are plain torch -- projections, norm + RoPE (tests/_norm_rope_restate.py), the soft mixture as the launches recorded from
the call under test (tests/_attn_restate.py: the coreset ranking and the sliding tables are constants of the backward), the
output projections -- and whose routers are softmax(linear(silu(temb))) on that model's own timestep embedding.  In float64
on the CPU it is the truth of the router gradients, in the 16-bit dtype it is the yardstick (torch's own autograd, one
rounding per operator).  The mini Wan block keeps its `.float()` calls in the float64 copy: fp32 roundings, four orders of
magnitude below the 16-bit errors that are measured against it.

The helpers that do not depend on a geometry come from tests/test_hip_processors_grad.py (imported, not restated)."""
import torch
import torch.nn.functional as F

import _mini_diffusers as M
import test_hip_processors_grad as G
from _norm_rope_restate import norm_rope

RecordLaunches = G._RecordLaunches  # per soft-mixture call, in call order: (launches, the three expert buffers)


def blocks_of(model):
    if hasattr(model, "blocks"):
        return list(model.blocks)
    return list(model.transformer_blocks) + list(model.single_transformer_blocks)


def embedder_of(model):
    if hasattr(model, "blocks"):
        return model.condition_embedder.time_embedder
    return model.time_text_embed.timestep_embedder


def _heads(x, H):  # (N, H*128) -> (H, N, 128)
    return x.view(x.shape[0], H, 128).transpose(0, 1)


class _Scores:
    """the (B, H, 3) scores of every layer of the running forward of a twin, from its own timestep embedding"""

    def __init__(self, twin):
        self.routers = [b.router for b in blocks_of(twin)]
        self.layers = []
        embedder_of(twin).register_forward_hook(self._hook)

    def _hook(self, module, args, temb):
        self.layers = []
        for r in self.routers:
            w, b = r.linear.weight, r.linear.bias
            self.layers.append(torch.softmax(F.linear(F.silu(temb.to(w.dtype)), w, b).view(temb.shape[0], r.heads, 3), dim=-1))


class _HunyuanRestated:
    def __init__(self, scores, layer, recorded):
        self.scores, self.layer, self.recorded = scores, layer, recorded

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, image_rotary_emb=None):
        H, dual = attn.heads, attn.add_q_proj is not None
        x, e = hidden_states[0], encoder_hidden_states[0]
        S, T = x.shape[0], e.shape[0]
        valid = int(attention_mask.reshape(-1, attention_mask.shape[-1])[0].sum())  # video + valid text keys
        cos, sin = image_rotary_emb
        if not dual:
            x = torch.cat([x, e], dim=0)
        q, k, v = (_heads(lin(x), H) for lin in (attn.to_q, attn.to_k, attn.to_v))
        q = norm_rope(q, attn.norm_q.weight, attn.norm_q.eps, cos, sin, S)
        k = norm_rope(k, attn.norm_k.weight, attn.norm_k.eps, cos, sin, S)
        if dual:
            eq, ek, ev = (_heads(lin(e), H) for lin in (attn.add_q_proj, attn.add_k_proj, attn.add_v_proj))
            eq = norm_rope(eq, attn.norm_added_q.weight, attn.norm_added_q.eps)
            ek = norm_rope(ek, attn.norm_added_k.weight, attn.norm_added_k.eps)
            q, k, v = torch.cat([q, eq], dim=1), torch.cat([k, ek], dim=1), torch.cat([v, ev], dim=1)
        if self.recorded is None:  # the dense teacher
            o = G._dense(q, k, v, valid)
        else:
            o = G._mixture(q, k, v, self.scores.layers[self.layer], *self.recorded[self.layer])
        o = o.transpose(0, 1).reshape(S + T, H * 128)
        hid, enc = o[:S], o[S:]
        if dual:
            hid, enc = attn.to_out[0](hid), attn.to_add_out(enc)
        return hid[None], enc[None]


class _WanRestated:
    """self attention of layer `layer` (the soft mixture), or with layer None the text cross attention (dense)"""

    def __init__(self, scores, layer, recorded):
        self.scores, self.layer, self.recorded = scores, layer, recorded

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, rotary_emb=None):
        H = attn.heads
        x = hidden_states[0]
        e = x if encoder_hidden_states is None else encoder_hidden_states[0]
        q, k, v = _heads(attn.to_q(x), H), _heads(attn.to_k(e), H), _heads(attn.to_v(e), H)
        cos = sin = None
        if rotary_emb is not None:  # the fp32 table the kernel is given (vorta_amd/attention/wan.py _cos_sin)
            f = rotary_emb.reshape(-1, rotary_emb.shape[-1])
            cos, sin = f.real.float().repeat_interleave(2, dim=1), f.imag.float().repeat_interleave(2, dim=1)
        n = 0 if cos is None else x.shape[0]
        q = norm_rope(q, attn.norm_q.weight, attn.norm_q.eps, cos, sin, rope_tokens=n, across_heads=True)
        k = norm_rope(k, attn.norm_k.weight, attn.norm_k.eps, cos, sin, rope_tokens=n, across_heads=True)
        if self.layer is None or self.recorded is None:
            o = G._dense(q, k, v)
        else:
            o = G._mixture(q, k, v, self.scores.layers[self.layer], *self.recorded[self.layer])
        return attn.to_out[0](o.transpose(0, 1).reshape(x.shape[0], H * 128))[None]


def restated_twin(model, recorded, dtype, device):
    """(twin, scores): the model's class and weights in `dtype` on `device` with restated attention; `recorded`: per layer
    what RecordLaunches kept of the call under test, or None for the dense teacher.  `scores.layers` holds the routers'
    output of the twin's latest forward."""
    from vorta_amd.patch.router import Router
    twin = type(model)()
    for b in blocks_of(twin):
        b.router = Router(embedding_dim=M.INNER, heads=M.H)
    twin.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    twin.to(device=device, dtype=dtype)
    scores = _Scores(twin)
    for layer, b in enumerate(blocks_of(twin)):
        if hasattr(b, "attn1"):
            b.attn1.set_processor(_WanRestated(scores, layer, recorded))
            b.attn2.set_processor(_WanRestated(scores, None, None))
        else:
            b.attn.set_processor(_HunyuanRestated(scores, layer, recorded))
    return twin, scores


def cast_inputs(inp, dtype, device):
    """the inputs of the call under test for a twin: floating tensors of the model's dtype become `dtype`; the timestep and
    the text mask keep theirs"""
    out = {}
    for k, v in inp.items():
        v = v.detach().to(device)
        out[k] = v.to(dtype) if v.is_floating_point() and k not in ("timestep", "encoder_attention_mask") else v
    return out


def training_loss(sample, scores, cot, acc):
    """a fixed cotangent on the output plus the reference's regulariser, mean(scores[..., 0] ** 2) per layer, summed in `acc`"""
    return (sample.to(acc) * cot.to(device=sample.device, dtype=acc)).sum() + sum((s[..., 0].to(acc) ** 2).mean() for s in scores)


def router_parameters(model):
    """name -> parameter, weight and bias of every layer's router"""
    return {f"layer {i} router {n}": p for i, b in enumerate(blocks_of(model))
            for n, p in (("weight", b.router.linear.weight), ("bias", b.router.linear.bias))}


def reference_gradients(model, inp, recorded, cot, dtype, device):
    """router gradients (name -> tensor) and the output of the restated twin in `dtype` on `device`"""
    twin, scores = restated_twin(model, recorded, dtype, device)
    sample = twin(**cast_inputs(inp, dtype, device), return_dict=False)[0]
    acc = torch.float64 if dtype == torch.float64 else torch.float32
    params = router_parameters(twin)
    grads = torch.autograd.grad(training_loss(sample, scores.layers, cot, acc), list(params.values()))
    return dict(zip(params, grads)), sample.detach()
