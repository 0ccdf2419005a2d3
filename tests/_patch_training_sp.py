"""Workers of tests/test_hip_patch_training_sp.py: what the gloo ranks that share the one GPU run (spawned processes import
this module), and the float64 truth rank 0 computes from what the ranks recorded.

Models, inputs and loss: tests/test_hip_patch_training.py (its builders, imported).  Recorder and `globalize`:
tests/_sp_soft_mixture.py.  Truth: tests/_patch_training_restate.py -- the restated whole model fed the launches of all ranks
in global coordinates, differentiated by torch in float64 (the truth) and in the model's 16-bit dtype (the yardstick).  Rank
set-up and spawn: tests/test_hip_sp_soft_mixture.py."""
import contextlib

import torch
import torch.nn.functional as F
from torch import nn
from torch.utils.checkpoint import checkpoint

import _mini_diffusers as M
import _patch_training_restate as R
import _sp_soft_mixture as C

# "even": the geometry of tests/test_hip_patch_training.py (192 tokens: 96 per rank of 2, 48 per rank of 4).  "odd": three
# latent frames, which 2 does not divide, 144 tokens, which it does -- tile, window and group of
# tests/test_hip_patch.py::test_hunyuan_pipeline_token_shard_takes_any_frame_count, which `RoutedGeometry` accepts.
GEOMS = {"even": dict(latent=(4, 6, 8), tile=(2, 3, 4), window=(3, 3, 3), group=(2, 3, 2)),
         "odd": dict(latent=(3, 6, 8), tile=(1, 3, 4), window=(3, 3, 3), group=(3, 3, 2))}
T_TEXT, T_VALID = 16, 11
INPUT_LEAVES = ("hidden_states", "encoder_hidden_states")
FID_FIELDS = ("sq_ref", "max_ref", "sq_err", "max_err")
COLLECTIVES = ("all_to_all_single", "all_to_all", "all_gather", "all_gather_into_tensor", "all_reduce", "reduce_scatter",
               "reduce_scatter_tensor", "broadcast", "batch_isend_irecv", "isend", "irecv", "send", "recv")


def kwargs_of(family, geom):
    from vorta.patch.utils import prepare_hunyuan_self_attn_kwargs, prepare_wan_self_attn_kwargs
    prepare = prepare_hunyuan_self_attn_kwargs if family == "hunyuan" else prepare_wan_self_attn_kwargs
    return prepare(dict(latent_shape=geom["latent"], window_size=geom["window"], tile_size=geom["tile"],
                        lowres_window_size=geom["group"], lowres_reduction_rate=0.5), C.dev())


def inputs_of(family, dtype, latent, seed=1):
    """tests/test_hip_patch_training.py `_inputs` at any latent: the same tensors on every rank (one device, one seed)"""
    g = torch.Generator(device=C.dev()).manual_seed(seed)
    hidden = torch.randn((1, 4) + tuple(latent), device=C.dev(), generator=g).to(dtype)
    if family == "wan":
        return dict(hidden_states=hidden, timestep=torch.tensor([412.0], device=C.dev()),
                    encoder_hidden_states=torch.randn((1, 20, 24), device=C.dev(), generator=g).to(dtype))
    mask = torch.zeros((1, T_TEXT), device=C.dev())
    mask[:, :T_VALID] = 1
    return dict(hidden_states=hidden, timestep=torch.tensor([637.0], device=C.dev()),
                encoder_hidden_states=torch.randn((1, T_TEXT, 24), device=C.dev(), generator=g).to(dtype),
                encoder_attention_mask=mask, pooled_projections=torch.randn((1, 16), device=C.dev(), generator=g).to(dtype),
                guidance=torch.tensor([6000.0], device=C.dev()).to(dtype))


def cotangent_of(dtype, latent):
    return torch.randn((1, 4) + tuple(latent), generator=torch.Generator().manual_seed(17)).to(dtype).to(C.dev())


def frames_of(x, rank, P):
    """this rank's latent frames of a (1, C, F, H, W) tensor: its contiguous chunk of the token sequence"""
    f = x.shape[2] // P
    return x[:, :, rank * f:(rank + 1) * f].contiguous()


def reference(model, inp, recorded, cot, dtype, device):
    """tests/_patch_training_restate.py `reference_gradients` with the latent and the text as further leaves: gradients of
    the router weights and biases and of `INPUT_LEAVES` (name -> tensor), and the output, of the restated twin in `dtype` on
    `device`"""
    twin, scores = R.restated_twin(model, recorded, dtype, device)
    x = R.cast_inputs(inp, dtype, device)
    for name in INPUT_LEAVES:
        x[name] = x[name].clone().requires_grad_(True)
    sample = twin(**x, return_dict=False)[0]
    acc = torch.float64 if dtype == torch.float64 else torch.float32
    params = R.router_parameters(twin)
    grads = torch.autograd.grad(R.training_loss(sample, scores.layers, cot, acc),
                                list(params.values()) + [x[name] for name in INPUT_LEAVES])
    return dict(zip(list(params) + list(INPUT_LEAVES), grads)), sample.detach()


def _step(model, local, kw, cot_local, P, cm):
    """one training forward on this rank and the two parts of its loss: the cotangent on what this rank is handed back,
    and the reference's regulariser -- computed identically on every rank, so the caller divides it by P"""
    from vorta.patch import routing_scores_of
    x = dict(local, **{name: local[name].detach().clone().requires_grad_(True) for name in INPUT_LEAVES})
    with cm:
        out = model(**x, return_dict=False, self_attention_kwargs=kw, return_routing_scores=True)
    scores = routing_scores_of(model)
    video = (out[0].float() * cot_local.float()).sum()
    reg = sum((s[..., 0].float() ** 2).mean() for s in scores)
    return x, out, scores, video + reg / P, video


def _fid_np(fid):
    return {n: getattr(fid, n).detach().float().cpu().numpy() for n in FID_FIELDS}


def model_worker(rank, world, port, ret, family, dtype_name, mode, geom_name, extras):
    """A whole patched mini model on `world` ranks.  mode "frame": every rank passes its latent frames and takes the loss on
    its output frames; "token": whole latents inside `token_sharded(model)`, the same loss on the whole output.
    extras: "checkpoint" (every block under a non-reentrant checkpoint, a teacher forward between forward and backward),
    "fidelity" (`expert_fidelity` of the same forward), "refuse_frames" (the frame-sharded call of this geometry)."""
    import test_hip_patch_training as PT
    import test_hip_sp_soft_mixture as SM
    dist, SP = SM._setup(rank, world, port)
    from vorta.patch import (all_reduce_router_grads, expert_fidelity, fidelity_of, original_attention, token_sharded)
    from vorta_amd import routed, set_attention_backward
    from vorta_amd.attention._sp import mixture_head_range
    previous = routed._attention_backward
    set_attention_backward("deterministic")
    try:
        dtype, geom, P = PT.DTYPES[dtype_name], GEOMS[geom_name], world
        model = PT._model(family, dtype)
        kw = kwargs_of(family, geom)
        inp = inputs_of(family, dtype, geom["latent"])
        cot = cotangent_of(dtype, geom["latent"])
        L, H = len(R.blocks_of(model)), M.H
        h0, h1 = mixture_head_range(H)
        mine = torch.zeros(H, dtype=torch.bool, device=C.dev())
        mine[h0:h1] = True
        res = {}
        if "refuse_frames" in extras:  # the caller cannot even cut this latent into frame shards: whatever it passes
            try:
                model(**dict(inp, hidden_states=inp["hidden_states"][:, :, :geom["latent"][0] // P + 1].contiguous()),
                      return_dict=False, self_attention_kwargs=kw)
                res["refusal"] = "not refused"
            except ValueError as e:
                res["refusal"] = str(e)
        token = mode == "token"
        local = inp if token else dict(inp, hidden_states=frames_of(inp["hidden_states"], rank, P))
        cot_local = cot if token else frames_of(cot, rank, P)
        inside = lambda check=False: token_sharded(model, check=check) if token else contextlib.nullcontext()  # noqa: E731
        one = None
        if rank == 0:  # the single-process forward of the same model, for the forward bound
            SP._enabled, SP._sp_size = False, 1
            with torch.no_grad():
                one = model(**inp, return_dict=False, self_attention_kwargs=kw)[0]
            SP._enabled, SP._sp_size = True, P
        with C.RecordSp() as rec:
            x, out, scores, loss, video = _step(model, local, kw, cot_local, P, inside(check=True))
        assert len(rec.calls) == L, (len(rec.calls), L)
        d_sc = torch.autograd.grad(video, scores, retain_graph=True)[0][:, 0]  # (L, H, 3), without the regulariser's share
        zeros_ok = bool((d_sc[:, ~mine] == 0).all()) and bool((d_sc[:, mine] != 0).any())
        loss.backward()
        torch.cuda.synchronize()
        params = R.router_parameters(model)
        missing = [n for n, p in params.items() if p.grad is None]
        pre = {n: p.grad.clone() for n, p in params.items() if p.grad is not None}
        pre.update({name: x[name].grad.clone() for name in INPUT_LEAVES})
        all_reduce_router_grads(model, op="sum")  # (raises, naming it, where a router has no gradient)
        post = {n: p.grad.clone() for n, p in params.items()}
        with inside(), torch.no_grad():
            plain = model(**local, return_dict=False, self_attention_kwargs=kw)[0]
        piece = dict(launches=[C.globalize(c, h0) for c in rec.calls], out=SM._np(out[0]), plain=SM._np(plain),
                     hidden_grad=SM._np(pre["hidden_states"]), text_grad=SM._np(pre["encoder_hidden_states"]), post={n: SM._np(g) for n, g in post.items()},
                     zeros_ok=zeros_ok, missing=missing, same_as_no_grad=bool(torch.equal(plain, out[0])))
        got = SM._gather(dist, piece)
        per_rank = {}
        if "checkpoint" in extras:
            blocks = R.blocks_of(model)
            for b in blocks:
                b.forward = lambda *a, _f=b.forward, **k: checkpoint(_f, *a, use_reentrant=False, **k)
            try:
                x2, out2, _, loss2, _ = _step(model, local, kw, cot_local, P, inside())
                with inside(), original_attention(model), torch.no_grad():  # a new entry: the student keeps its own mode
                    teacher = model(**local, return_dict=False)[0]
                leaves = list(params.values()) + [x2[name] for name in INPUT_LEAVES]
                passes = [torch.autograd.grad(loss2, leaves, retain_graph=True) for _ in range(2)]
                torch.cuda.synchronize()
            finally:
                for b in blocks:
                    del b.forward
            names = list(params) + list(INPUT_LEAVES)
            per_rank["checkpoint"] = dict(
                out_equal=bool(torch.equal(out2[0], out[0])), teacher_differs=not torch.equal(teacher, out[0].detach()),
                teacher_shape=tuple(teacher.shape),
                differ_from_unchecked=[n for n, g in zip(names, passes[0]) if not torch.equal(g, pre[n])],
                differ_between_passes=[n for n, a, b in zip(names, passes[0], passes[1]) if not torch.equal(a, b)])
            del loss2, passes, out2, x2
        if "fidelity" in extras:
            with inside(), expert_fidelity(model), torch.no_grad():
                measured = model(**local, return_dict=False, self_attention_kwargs=kw)[0]
            fid = fidelity_of(model)  # a collective: every rank
            per_rank["fidelity"] = dict(values=_fid_np(fid), shapes=[tuple(getattr(fid, n).shape) for n in FID_FIELDS],
                                        out_same=bool(torch.equal(measured, plain)))
        if rank == 0:
            t = lambda a: torch.as_tensor(a).to(C.dev())  # noqa: E731
            recorded = [C.as_launches([c for g in got for c in g["launches"][layer]]) for layer in range(L)]
            ref, o64 = reference(model, inp, recorded, cot, torch.float64, "cpu")
            t16, _ = reference(model, inp, recorded, cot, dtype, C.dev())
            if token:
                sample = t(got[0]["out"])
                hidden_grad = sum(t(g["hidden_grad"]).double() for g in got)
            else:
                sample = torch.cat([t(g["out"]) for g in got], dim=2)
                hidden_grad = torch.cat([t(g["hidden_grad"]) for g in got], dim=2)
            total = {n: t(a) for n, a in got[0]["post"].items()}
            total["hidden_states"] = hidden_grad
            # the text: a Hunyuan rank holds the WHOLE gradient (the text stream carries whole cotangents between the
            # layers, patch/_engine.py `_SumOverRanks`), a Wan rank its share (cross attention of its own queries)
            text_sum = sum(t(g["text_grad"]).double() for g in got)
            total["encoder_hidden_states"] = t(got[0]["text_grad"]) if family == "hunyuan" else text_sum
            other = text_sum if family == "hunyuan" else t(got[0]["text_grad"])
            res.update(
                layers=L, names=list(ref), missing=[n for g in got for n in g["missing"]],
                zeros_ok=all(g["zeros_ok"] for g in got), same_as_no_grad=all(g["same_as_no_grad"] for g in got),
                ranks_agree_after_reduce=all(all((g["post"][n] == got[0]["post"][n]).all() for n in got[0]["post"]) for g in got),
                plain_equal_on_every_rank=(not token) or all((g["plain"] == got[0]["plain"]).all() for g in got),
                out_shape=tuple(got[0]["out"].shape),
                text_grad_equal_on_every_rank=all((g["text_grad"] == got[0]["text_grad"]).all() for g in got),
                text_grad_other_reading=C.rel_err(other.cpu(), ref["encoder_hidden_states"]),
                fwd=(C.rel_err(sample.cpu(), o64), C.rel_err(one.cpu(), o64)),
                bwd={n: (C.rel_err(total[n].cpu(), ref[n]), C.rel_err(t16[n].cpu(), ref[n])) for n in ref})
            ret["res"] = res
        ret[f"rank {rank}"] = per_rank
    finally:
        routed._attention_backward = previous
    dist.barrier()
    SP.cleanup()


# ------------------------------------------------------------------------------------------------- Wan cross attention
class WanCrossAttn(nn.Module):
    """the cross attention of a Wan block (`attn2`): RMSNorm across all H * 128 channels, text keys of another width's
    projection; `image`: the I2V branch as well (add_k_proj / add_v_proj / norm_added_k on the first 257 tokens)"""
    H, WIDTH = 6, 64

    def __init__(self, image, dtype, seed):
        super().__init__()
        torch.manual_seed(seed)
        H, D, W = self.H, 128, self.WIDTH
        self.heads = H
        self.to_q, self.to_k, self.to_v = (nn.Linear(W, H * D) for _ in range(3))
        self.norm_q, self.norm_k = nn.RMSNorm(H * D, eps=1e-6), nn.RMSNorm(H * D, eps=1e-6)
        self.add_k_proj = self.add_v_proj = self.norm_added_k = None
        if image:
            self.add_k_proj, self.add_v_proj = nn.Linear(W, H * D), nn.Linear(W, H * D)
            self.norm_added_k = nn.RMSNorm(H * D, eps=1e-6)
        self.to_out = nn.ModuleList([nn.Linear(H * D, W), nn.Identity()])
        for m in self.modules():
            if isinstance(m, nn.RMSNorm):
                nn.init.uniform_(m.weight, 0.5, 1.5)
        self.to(C.dev()).to(dtype)


CROSS_WANTED = ("hidden", "enc", "to_q.weight", "to_k.weight", "to_v.weight", "to_out.0.weight", "add_k_proj.weight",
                "add_v_proj.weight", "norm_q.weight", "norm_k.weight", "norm_added_k.weight")


def wan_cross_restated(Pm, hidden, enc, image):
    """vorta_amd/attention/wan.py for `encoder_hidden_states is not None`, in torch: no rotation, two dense attentions whose
    outputs add in front of the output projection"""
    import test_hip_processors_grad as G
    from _norm_rope_restate import norm_rope
    lin = lambda n, x: F.linear(x, Pm[n + ".weight"], Pm[n + ".bias"])  # noqa: E731
    x, e = hidden[0], enc[0]
    e_img = None
    if image:
        e_img, e = e[:257], e[257:]
    q = norm_rope(G._heads(lin("to_q", x)), Pm["norm_q.weight"], 1e-6, across_heads=True)
    k = norm_rope(G._heads(lin("to_k", e)), Pm["norm_k.weight"], 1e-6, across_heads=True)
    o = G._dense(q, k, G._heads(lin("to_v", e)))
    if image:  # (the processor runs the module's own RMSNorm here, before the head split)
        k_img = F.rms_norm(lin("add_k_proj", e_img), (Pm["norm_added_k.weight"].shape[0],), Pm["norm_added_k.weight"], 1e-6)
        o_img = G._dense(q, G._heads(k_img), G._heads(lin("add_v_proj", e_img)))
        return lin("to_out.0", o.transpose(0, 1).reshape(x.shape[0], -1) + o_img.transpose(0, 1).reshape(x.shape[0], -1))[None]
    return lin("to_out.0", o.transpose(0, 1).reshape(x.shape[0], -1))[None]


def wan_cross_worker(rank, world, port, ret, dtype_name):
    """`WanAttnProcessor2_0(differentiable=True)` with `encoder_hidden_states` on this rank's query shard, in grad mode
    under sequence parallelism: text only, and text behind 257 image tokens.  Every collective of torch.distributed is
    counted from the first processor call to the end of the backward."""
    import test_hip_patch_training as PT
    import test_hip_processors_grad as G
    import test_hip_sp_soft_mixture as SM
    dist, SP = SM._setup(rank, world, port)
    from vorta_amd import routed, set_attention_backward
    from vorta_amd.attention import WanAttnProcessor2_0
    previous = routed._attention_backward
    set_attention_backward("deterministic")
    try:
        dtype, P = PT.DTYPES[dtype_name], world
        S, W = G.S, WanCrossAttn.WIDTH
        Sl = S // P
        proc = WanAttnProcessor2_0(differentiable=True)
        for image in (False, True):
            attn = WanCrossAttn(image, dtype, seed=51 + image)
            gen = torch.Generator().manual_seed(23 + image)
            hidden = torch.randn((1, S, W), generator=gen).to(dtype).to(C.dev())
            enc = torch.randn((1, 40 + (257 if image else 0), W), generator=gen).to(dtype).to(C.dev())
            cot = torch.randn((1, S, W), generator=gen).to(dtype).to(C.dev())
            calls = {}
            stock = {name: getattr(dist, name) for name in COLLECTIVES if hasattr(dist, name)}

            def counted(name, fn):
                def wrapper(*a, **k):
                    calls[name] = calls.get(name, 0) + 1
                    return fn(*a, **k)
                return wrapper
            for name, fn in stock.items():
                setattr(dist, name, counted(name, fn))
            try:
                h = hidden[:, rank * Sl:(rank + 1) * Sl].clone().requires_grad_(True)
                e = enc.clone().requires_grad_(True)
                with torch.no_grad():
                    plain = proc(attn, h.detach(), enc, None, None)
                out = proc(attn, h, e, None, None)
                (out * cot[:, rank * Sl:(rank + 1) * Sl]).sum().backward()
                torch.cuda.synchronize()
            finally:
                for name, fn in stock.items():
                    setattr(dist, name, fn)
            grads = {"hidden": SM._np(h.grad), "enc": SM._np(e.grad)}
            grads.update({n: SM._np(p.grad) for n, p in attn.named_parameters() if p.grad is not None})
            got = SM._gather(dist, dict(grads=grads, out=SM._np(out), calls=calls, requires_grad=bool(out.requires_grad),
                                        bits=bool(torch.equal(out, plain))))
            if rank == 0:
                t = lambda a: torch.as_tensor(a).to(C.dev())  # noqa: E731
                total = {n: (torch.cat([t(g["grads"][n]) for g in got], dim=1).double() if n == "hidden"
                             else sum(t(g["grads"][n]).double() for g in got)) for n in got[0]["grads"]}

                def ref(dt):
                    Pm = {n: p.detach().to(dt).requires_grad_(True) for n, p in attn.named_parameters()}
                    Lv = {"hidden": hidden.detach().to(dt).requires_grad_(True), "enc": enc.detach().to(dt).requires_grad_(True)}
                    o = wan_cross_restated(Pm, Lv["hidden"], Lv["enc"], image)
                    names = [n for n in CROSS_WANTED if n in Lv or n in Pm]
                    g = torch.autograd.grad((o * cot.to(dt)).sum(), [dict(Lv, **Pm)[n] for n in names])
                    return dict(zip(names, g)), o.detach()

                r64, o64 = ref(torch.float64)
                r16, o16 = ref(dtype)
                sample = torch.cat([t(g["out"]) for g in got], dim=1)
                ret["image" if image else "text"] = dict(
                    calls=[g["calls"] for g in got], bits=[g["bits"] for g in got], graph=[g["requires_grad"] for g in got],
                    missing=[n for n in r64 if n not in total], fwd=(C.rel_err(sample, o64), C.rel_err(o16, o64)),
                    bwd={n: (C.rel_err(total[n], r64[n]), C.rel_err(r16[n], r64[n])) for n in r64 if n in total})
    finally:
        routed._attention_backward = previous
    dist.barrier()
    SP.cleanup()
