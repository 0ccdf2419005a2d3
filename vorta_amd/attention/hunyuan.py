"""HunyuanVideo (MMDiT: video + text tokens in one sequence) attention processors.

Same classes, call protocol and keyword names as vorta/attention/hunyuan.py, so diffusers' `Attention.forward`
and the patched block forwards (modeling_hunyuan.py:492-499,556-563) can call them unchanged.  Projections, qk
RMSNorm and RoPE stay in torch (rocBLAS); everything between post-RoPE q,k,v and the output projection runs in
libvorta_hip.so (vorta_amd/routed.py).
"""
from typing import List, Optional, Tuple

import torch

from .. import ops
from .. import torch_ops as _torch_ops  # registers torch.ops.vorta.*: what the processors launch through
from ..routed import (HeadRouting, dense_attention_autograd, geometry_for, qk_norm_rope_autograd,
                      soft_mixture_attention_autograd)
from ..ulysses import SP_STATE, shrink_dim
from ._eval import check_eval_input, launch_routes, refuse_under_sequence_parallel, resolve_routes
from .coreset_select import LowresGroupInfo
from .sliding_tile import SlidingTileDescriptor


def apply_rotary_emb(x: torch.Tensor, freqs_cis: Tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
    """Rotary embedding on (B,H,S,D) with (cos, sin) of shape (S,D), interleaved real/imag pairs.
    [ext] restates diffusers==0.33.1 `apply_rotary_emb(use_real=True, use_real_unbind_dim=-1)`, which the
    reference imports (hunyuan.py:18,97-98); it sits before the attention boundary."""
    cos, sin = freqs_cis
    cos, sin = cos[None, None].to(x.device), sin[None, None].to(x.device)
    x_real, x_imag = x.reshape(*x.shape[:-1], -1, 2).unbind(-1)
    x_rot = torch.stack([-x_imag, x_real], dim=-1).flatten(3)
    return (x.float() * cos + x_rot.float() * sin).to(x.dtype)


def _fusable_norm(norm, x: torch.Tensor, numel: int) -> bool:
    """can vorta_qk_norm_rope stand in for this module?  (RMSNorm with an `eps` and an optional `weight` of the
    expected size, half-precision CUDA input)"""
    if norm is None or not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16) or x.shape[-1] != 128:
        return False
    if "RMSNorm" not in type(norm).__name__ or getattr(norm, "eps", None) is None:
        return False
    w = getattr(norm, "weight", None)
    return w is None or w.numel() == numel


def fused_norm_rope(x: torch.Tensor, norm, rope: Optional[Tuple[torch.Tensor, torch.Tensor]], rope_tokens: int = 0):
    """RMSNorm (+ RoPE on the first `rope_tokens` tokens) of a (1,H,N,D) projection view, in place, in one HIP
    kernel (hunyuan.py:62-104 are two module calls and ~10 elementwise passes)."""
    w = getattr(norm, "weight", None)
    cos, sin = rope if rope is not None else (None, None)
    torch.ops.vorta.qk_norm_rope(x[0], w, float(norm.eps), cos, sin, rope_tokens if rope is not None else 0)
    return x


def fused_norm_rope_grad(x: torch.Tensor, norm, rope: Optional[Tuple[torch.Tensor, torch.Tensor]], rope_tokens: int = 0):
    """`fused_norm_rope` for a training graph: out of place (a contiguous copy of x), differentiable in x and the norm's
    weight (routed.qk_norm_rope_autograd: one HIP pass forward, one backward)."""
    cos, sin = rope if rope is not None else (None, None)
    return qk_norm_rope_autograd(x, getattr(norm, "weight", None), float(norm.eps), cos, sin,
                                 rope_tokens if rope is not None else 0)


# project video and text tokens straight into ONE (1, S+T, H*D) buffer per tensor: the `torch.cat([q, eq], dim=2)` of a
# dual-stream block (hunyuan.py:106-134: a read and a write of all of q, k and v) and the input concat of a
# single-stream block (hunyuan.py:47-48) disappear (SURVEY.md §8f N1 "+ text concat").  VORTA_DEBUG=joint_projection=0: the
# reference's route (A/B, tests).
JOINT_PROJECTION = __import__("vorta_amd._debug", fromlist=["flag"]).flag("joint_projection", "1") != "0"


def _linear_into(lin: torch.nn.Linear, x2d: torch.Tensor, dst: torch.Tensor) -> None:
    """dst (rows, out_features; contiguous rows of a larger buffer) = lin(x2d), written by the GEMM itself"""
    if lin.bias is not None:
        torch.addmm(lin.bias, x2d, lin.weight.t(), out=dst)
    else:
        torch.mm(x2d, lin.weight.t(), out=dst)


def _joint_projectable(x: torch.Tensor, e: torch.Tensor, lins, grad: bool = False) -> bool:
    """grad=True: would the inference call of these modules on these inputs take the joint projection?  (asked by the
    training forward, which cannot use `out=` but projects the same row ranges, for the same bits)"""
    if not JOINT_PROJECTION or x.shape[0] != 1 or not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float16):
        return False
    if e.dtype != x.dtype or not all(type(m) is torch.nn.Linear and m.weight.dtype == x.dtype for m in lins):
        return False
    # writing through lin.weight bypasses Linear.forward: only when nothing hangs on that forward (accelerate's offload
    # hooks keep the weights on meta / CPU until it runs; user hooks would be skipped)
    if any(m.weight.device != x.device or hasattr(m, "_hf_hook") or m._forward_hooks or m._forward_pre_hooks for m in lins):
        return False
    # `out=` is an inference-only form: autograd refuses it as soon as an argument requires grad
    return grad or not (torch.is_grad_enabled() and (x.requires_grad or e.requires_grad or
                                                     any(m.weight.requires_grad for m in lins)))


def _valid_keys(attention_mask: torch.Tensor) -> torch.Tensor:
    """Number of valid keys L (int32, shape (1,), on the device) from the reference's attention mask
    (hunyuan.py:169 `attention_mask.squeeze().sum()` on the diffusers 0.33 [B,1,1,N] key mask).  Other diffusers versions
    hand a [B,N,N] / [B,1,N,N] mask: one query row is reduced then, anything else is refused instead of silently
    attending padded text."""
    N = attention_mask.shape[-1]
    rows = attention_mask.numel() // (attention_mask.shape[0] * N)
    if rows not in (1, N):
        raise ValueError(f"unsupported attention_mask shape {tuple(attention_mask.shape)}: expected [B,1,1,N] or [B,(1,)N,N]")
    row = attention_mask.reshape(attention_mask.shape[0], rows, N)[0, 0]
    return row.sum(dtype=torch.int32).reshape(1)


class HunyuanVideoFlashAttnProcessor:
    """Dense attention for every head: the --native_attention path (hunyuan.py:35-238).

    `differentiable=True` (off by default): a call in grad mode builds an autograd graph from the output back to
    hidden_states, encoder_hidden_states and the module parameters -- projections through the modules, norm + RoPE through
    `qk_norm_rope_autograd`, attention through `dense_attention_autograd`.  Under torch.no_grad() such a processor takes
    the inference path and gives its bits."""

    _HAS_BACKWARD = True  # the concrete class can sit in a training graph (the Eval classes cannot: hard top-1)

    def __init__(self, differentiable: bool = False):
        ops._C.lib()  # fail loudly now if libvorta_hip.so is missing: there is no fallback path
        if differentiable and not type(self)._HAS_BACKWARD:
            raise ValueError(f"{type(self).__name__} routes every head to its top-1 expert, which has no gradient: "
                             "differentiable=True belongs to the dense and the soft-mixture (Train) processors")
        self.differentiable = bool(differentiable)

    def _grad_path(self, sequence_parallel: bool = False) -> bool:
        """build an autograd graph in this call?  `sequence_parallel`: the caller has a differentiable exchange (the soft
        mixture, attention/_sp.py); the dense attention has none -- the teacher runs under torch.no_grad()"""
        if not (self.differentiable and torch.is_grad_enabled()):
            return False
        if SP_STATE.enabled and not sequence_parallel:
            raise NotImplementedError("differentiable=True of the dense attention is not sequence-parallel in this build: "
                                      "only the soft mixture has a differentiable exchange")
        return True

    # -- steps 1-4 of hunyuan.py:42-134: everything before the attention boundary ----------------------
    def _project(self, attn, hidden_states, encoder_hidden_states, image_rotary_emb, grad: bool = False):
        """grad=True: every step stays visible to autograd -- no GEMM `out=`, no in-place kernel"""
        single_stream = attn.add_q_proj is None  # single blocks carry text inside hidden_states
        T = encoder_hidden_states.shape[1]
        rope = None
        if image_rotary_emb is not None:
            rope = (shrink_dim(image_rotary_emb[0], dim=0), shrink_dim(image_rotary_emb[1], dim=0))
        norm_rope = fused_norm_rope_grad if grad else fused_norm_rope
        joint = None if grad else self._project_joint(attn, hidden_states, encoder_hidden_states, rope, single_stream)
        if joint is not None:
            return (*joint, T)
        if single_stream and grad and self._joint_applies(attn, hidden_states, encoder_hidden_states, True, grad=True):
            # the inference call projects the video and the text rows in a GEMM each (_project_joint); one GEMM over the
            # concatenated rows rounds differently (seen in fp16).  The training forward gives the inference bits.
            q, k, v = (torch.cat([lin(hidden_states), lin(encoder_hidden_states)], dim=1).unflatten(2, (attn.heads, -1))
                       .transpose(1, 2) for lin in (attn.to_q, attn.to_k, attn.to_v))
        else:
            if single_stream:
                hidden_states = torch.cat([hidden_states, encoder_hidden_states], dim=1)
            q = attn.to_q(hidden_states).unflatten(2, (attn.heads, -1)).transpose(1, 2)
            k = attn.to_k(hidden_states).unflatten(2, (attn.heads, -1)).transpose(1, 2)
            v = attn.to_v(hidden_states).unflatten(2, (attn.heads, -1)).transpose(1, 2)
        n_video = q.shape[2] - (T if single_stream else 0)
        if q.shape[0] == 1 and _fusable_norm(attn.norm_q, q, 128) and _fusable_norm(attn.norm_k, k, 128):
            # one in-place HIP pass per tensor: norm everywhere, rotation on the video tokens only
            q = norm_rope(q, attn.norm_q, rope, n_video)
            k = norm_rope(k, attn.norm_k, rope, n_video)
        else:
            if attn.norm_q is not None:
                q = attn.norm_q(q)
            if attn.norm_k is not None:
                k = attn.norm_k(k)
            if rope is not None:
                if single_stream:
                    q = torch.cat([apply_rotary_emb(q[:, :, :-T], rope), q[:, :, -T:]], dim=2)
                    k = torch.cat([apply_rotary_emb(k[:, :, :-T], rope), k[:, :, -T:]], dim=2)
                else:
                    q, k = apply_rotary_emb(q, rope), apply_rotary_emb(k, rope)
        if not single_stream:
            eq = attn.add_q_proj(encoder_hidden_states).unflatten(2, (attn.heads, -1)).transpose(1, 2)
            ek = attn.add_k_proj(encoder_hidden_states).unflatten(2, (attn.heads, -1)).transpose(1, 2)
            ev = attn.add_v_proj(encoder_hidden_states).unflatten(2, (attn.heads, -1)).transpose(1, 2)
            if eq.shape[0] == 1 and _fusable_norm(attn.norm_added_q, eq, 128) and _fusable_norm(attn.norm_added_k, ek, 128):
                eq = norm_rope(eq, attn.norm_added_q, None)
                ek = norm_rope(ek, attn.norm_added_k, None)
            else:
                if attn.norm_added_q is not None:
                    eq = attn.norm_added_q(eq)
                if attn.norm_added_k is not None:
                    ek = attn.norm_added_k(ek)
            q, k, v = torch.cat([q, eq], dim=2), torch.cat([k, ek], dim=2), torch.cat([v, ev], dim=2)
        return q, k, v, T

    @staticmethod
    def _joint_applies(attn, hidden_states, encoder_hidden_states, single_stream: bool, grad: bool = False) -> bool:
        """do the modules and inputs allow `_project_joint`?  (grad=True: would they, in the inference call)"""
        vid = (attn.to_q, attn.to_k, attn.to_v)
        txt = vid if single_stream else (attn.add_q_proj, attn.add_k_proj, attn.add_v_proj)
        if not _joint_projectable(hidden_states, encoder_hidden_states, vid + txt, grad):
            return False
        H, out_f = attn.heads, attn.to_q.out_features
        probe = hidden_states.new_empty((1, H, 1, out_f // H))
        norms = (attn.norm_q, attn.norm_k) if single_stream else (attn.norm_q, attn.norm_k, attn.norm_added_q,
                                                                   attn.norm_added_k)
        if out_f // H != 128 or not all(_fusable_norm(n, probe, 128) for n in norms):
            return False
        return all(m.out_features == out_f for m in vid + txt)

    @staticmethod
    def _project_joint(attn, hidden_states, encoder_hidden_states, rope, single_stream: bool):
        """Fused-norm case: the video and text projections land in ONE (1, S+T, H*D) buffer per tensor, written by the
        GEMMs -- no `torch.cat([q, eq], dim=2)` pass over q, k, v in a dual-stream block (hunyuan.py:106-134), no concat
        of the block inputs in a single-stream one (hunyuan.py:47-48); qk-norm + RoPE run in place on the row ranges.
        None when the modules do not allow it (the caller then takes the reference's route)."""
        if not HunyuanVideoFlashAttnProcessor._joint_applies(attn, hidden_states, encoder_hidden_states, single_stream):
            return None
        vid = (attn.to_q, attn.to_k, attn.to_v)
        txt = vid if single_stream else (attn.add_q_proj, attn.add_k_proj, attn.add_v_proj)
        S_, T, H = hidden_states.shape[1], encoder_hidden_states.shape[1], attn.heads
        out_f = attn.to_q.out_features
        x2d, e2d = hidden_states[0], encoder_hidden_states[0]
        qkv = []
        for lin, elin in zip(vid, txt):
            buf = hidden_states.new_empty((1, S_ + T, out_f))
            _linear_into(lin, x2d, buf[0, :S_])
            _linear_into(elin, e2d, buf[0, S_:])
            qkv.append(buf.unflatten(2, (H, -1)).transpose(1, 2))  # (1, H, S+T, D) view
        q, k, v = qkv
        if single_stream:  # one norm for both row ranges, rotation on the video rows
            fused_norm_rope(q, attn.norm_q, rope, S_)
            fused_norm_rope(k, attn.norm_k, rope, S_)
        else:
            fused_norm_rope(q[:, :, :S_], attn.norm_q, rope, S_)
            fused_norm_rope(k[:, :, :S_], attn.norm_k, rope, S_)
            fused_norm_rope(q[:, :, S_:], attn.norm_added_q, None)
            fused_norm_rope(k[:, :, S_:], attn.norm_added_k, None)
        return q, k, v

    # -- step 6 (hunyuan.py:191-208) ---------------------------------------------------------------------
    @staticmethod
    def _output(attn, out_bshd: torch.Tensor, T: int):
        """out_bshd: (B, S+T, H, D) -- the kernels wrote it in this layout, so the head merge is a view."""
        hidden = out_bshd[:, :-T].flatten(2, 3)
        enc = out_bshd[:, -T:].flatten(2, 3)
        if getattr(attn, "to_out", None) is not None:
            hidden = attn.to_out[1](attn.to_out[0](hidden))
        if getattr(attn, "to_add_out", None) is not None:
            enc = attn.to_add_out(enc)
        return hidden, enc

    @staticmethod
    def _new_out(q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        B, H, N, D = q.shape
        buf = torch.empty((B, N, H, D), dtype=q.dtype, device=q.device)
        return buf, buf.permute(0, 2, 1, 3)  # (B,H,N,D) view for the kernels

    @staticmethod
    def _text_valid(attention_mask: torch.Tensor, T: int, descriptor=None) -> int:
        if descriptor is not None:
            return descriptor.text_seq_length_no_pad
        # the reference reads this on the host as well (hunyuan.py:169 `attention_mask.squeeze().sum()`).  The mask
        # spans [video | text]: the global video under the reference's patched forward (modeling_hunyuan.py:86-88),
        # the local shard under the stock diffusers forward -- either way its video part is all ones.
        return int(_valid_keys(attention_mask).item()) - (attention_mask.shape[-1] - T)

    def _dense(self, q, k, v, attention_mask, T):
        B = q.shape[0]
        assert B == 1, f"Batch size {B} is not supported for {self.__class__.__name__}."  # hunyuan.py:168
        if SP_STATE.enabled:
            from ._sp import sp_attention
            return sp_attention(q, k, v, T, None, None, model="hunyuan", attention_mask=attention_mask)
        buf, out = self._new_out(q)
        # L = attention_mask.sum() stays on the device: no host sync (the reference syncs at hunyuan.py:169)
        L = _valid_keys(attention_mask)
        N = q.shape[2]
        torch.ops.vorta.attn_fwd(q[0], k[0], v[0], out[0], N, N, q_valid=N, n_kv_dev=L, q_valid_dev=L)
        return buf

    def _dense_grad(self, q, k, v, attention_mask):
        """`_dense` behind autograd.  dense_attention_autograd takes the valid-key count as a host integer: read once here,
        as the reference does (hunyuan.py:169); the no-grad path keeps its sync-free form."""
        assert q.shape[0] == 1, f"Batch size {q.shape[0]} is not supported for {self.__class__.__name__}."
        L = min(max(int(_valid_keys(attention_mask).item()), 1), q.shape[2])
        out = dense_attention_autograd(q.contiguous(), k.contiguous(), v.contiguous(), kv_valid=L, q_valid=L)
        return out.transpose(1, 2)  # (B, S+T, H, D)

    @torch.no_grad()  # forward only
    def _call_no_grad(self, attn, hidden_states, encoder_hidden_states, attention_mask, image_rotary_emb):
        q, k, v, T = self._project(attn, hidden_states, encoder_hidden_states, image_rotary_emb)
        return self._output(attn, self._dense(q, k, v, attention_mask, T), T)

    def __call__(self, attn, hidden_states, encoder_hidden_states, attention_mask, image_rotary_emb):
        if not self._grad_path():  # the default: no autograd graph, whatever the inputs ask for
            return self._call_no_grad(attn, hidden_states, encoder_hidden_states, attention_mask, image_rotary_emb)
        q, k, v, T = self._project(attn, hidden_states, encoder_hidden_states, image_rotary_emb, grad=True)
        return self._output(attn, self._dense_grad(q, k, v, attention_mask), T)


class HunyuanVideoFlashAttnProcessorTripleEval(HunyuanVideoFlashAttnProcessor):
    """Inference-time routed attention: hard top-1 expert per head (hunyuan.py:516-661)."""

    _HAS_BACKWARD = False

    def __init__(self, check_input: bool = False, differentiable: bool = False):
        super().__init__(differentiable)
        self.check_input = check_input

    def _check_input(self, hidden_states, lowres_group_info, latent_shape, window_size, tile_size):
        """hunyuan.py:247-272: attention/_eval.py `check_eval_input`"""
        if not self.check_input:
            return
        check_eval_input(hidden_states, lowres_group_info, latent_shape, window_size, tile_size)

    @torch.no_grad()
    def __call__(self, attn, hidden_states, encoder_hidden_states, attention_mask, image_rotary_emb,
                 routing_score: torch.Tensor, tau_sparse: float,
                 lowres_group_info: Optional[LowresGroupInfo] = None,
                 flex_attn_mask_func: Optional[SlidingTileDescriptor] = None,
                 window_size: Tuple[int, int, int] = (3, 3, 3), tile_size: Tuple[int, int, int] = (6, 8, 8),
                 latent_shape: Tuple[int, int, int] = (30, 48, 80),
                 head_routing: Optional[HeadRouting] = None, experts_host: Optional[List[int]] = None,
                 fidelity: Optional[list] = None, fidelity_rows=None, fidelity_heads: str = "sparse",
                 expert_fidelity: Optional[list] = None, route_rule=None, route_sink: Optional[list] = None,
                 tier_routing: Optional[dict] = None, repair_above: Optional[float] = None,
                 repair_sink: Optional[list] = None):
        """Keyword names as hunyuan.py:521-539.  `head_routing` / `experts_host` are this build's additions: the
        routes of this layer already dispatched by the step's route plan (vorta_amd/patch/_engine.py), on the device /
        on the host; without them the dispatch runs here from `routing_score`.
        fidelity: a list that receives this call's `ops.SampledFidelity` -- the routed output as run against dense attention on
        `fidelity_rows` sampled video rows of the `fidelity_heads` (routed.routed_attention; under sequence parallelism the
        heads this rank holds, filed under their global ids: attention/_sp.py); None: the launches of today.
        expert_fidelity: a list that receives this call's `ops.ExpertFidelity` on the same `fidelity_rows` -- what every expert
        would have written for every head, and the routed rows (routed.sampled_expert_fidelity); refused by name under sequence
        parallelism.
        route_rule: a `routed.RouteRule`: the call is routed by its OWN measurement (routed.route_by_fidelity on the projected
        q, k, v: a stated error bound or FLOP budget, on the device, no host read); `routing_score`, `tau_sparse` and
        `head_routing` are then not consulted, and `route_sink` (a list) receives (expert_ids, lists, counts, fid).  Refused
        by name under sequence parallelism.  With `route_rule.covers_precision` under an 8-bit process precision the call is
        routed AND launched over (precision tier, expert) pairs (routed.route_by_fidelity(tiers=...), then
        routed.routed_attention_tiers on the operands the measurement prepared); the sink then receives a 5-tuple: expert_ids,
        the (n_tiers,3,H) lists, the (n_tiers,3) counts, the `native` tier's record, and a dictionary with `tiers` (names, in
        launch order), `tier_ids` (int32 (H,), global ids) and `fids` (tier -> record).
        tier_routing: tier -> HeadRouting (a stored `TierRoutes.routings`): the call launches it with
        routed.routed_attention_tiers; nothing else is consulted.  Refused by name under sequence parallelism.
        repair_above / repair_sink: the call VERIFIES what it launched on the `fidelity_rows` and re-runs every head further
        than `repair_above` from dense attention, dense in the input dtype, in this forward (routed.routed_attention_repaired):
        whether the routes come from `route_rule`, from a device `head_routing` (its `expert_ids`; derived from its lists where
        it has none) or from `tier_routing` -- then a routed.RepairableRoutes or TierRoutes, whose joint tables are rewritten in
        place, as a `head_routing`'s lists and counts are: a later call with the same tables launches the repaired heads dense.
        `repair_sink` (a list) receives the call's routed.RepairRecord; a `fidelity` sink receives that record's
        SampledFidelity: the rows as they were BEFORE the repair.  None: the launches of today.  Refused by name under sequence
        parallelism."""
        self._check_input(hidden_states, lowres_group_info, latent_shape, window_size, tile_size)
        q, k, v, T = self._project(attn, hidden_states, encoder_hidden_states, image_rotary_emb)
        assert q.shape[0] == 1, f"Batch size {q.shape[0]} is not supported for {self.__class__.__name__}."
        te = self._text_valid(attention_mask, T, flex_attn_mask_func)
        if SP_STATE.enabled:
            refuse_under_sequence_parallel(expert_fidelity, route_rule, tier_routing, repair_above)
            from ._sp import sp_attention
            buf = sp_attention(q, k, v, T, routing_score, tau_sparse, model="hunyuan", text_valid=te,
                               lowres_group_info=lowres_group_info, window_size=window_size, tile_size=tile_size,
                               latent_shape=latent_shape, experts_host=experts_host, fidelity=fidelity,
                               fidelity_rows=fidelity_rows, fidelity_heads=fidelity_heads)
            return self._output(attn, buf, T)
        geometry = _torch_ops.geometry_args(lowres_group_info, window_size, tile_size, latent_shape)
        routes = resolve_routes(q, k, v, geometry, model="hunyuan", text_len=T, text_valid=te, routing_score=routing_score,
                                tau_sparse=tau_sparse, head_routing=head_routing, route_rule=route_rule, route_sink=route_sink,
                                tier_routing=tier_routing)
        buf, out = self._new_out(q)
        launch_routes(q, k, v, out, routes, geometry, model="hunyuan", text_len=T, text_valid=te, fidelity=fidelity,
                      fidelity_rows=fidelity_rows, fidelity_heads=fidelity_heads, expert_fidelity=expert_fidelity,
                      repair_above=repair_above, repair_sink=repair_sink)
        return self._output(attn, buf, T)


class HunyuanVideoFlashAttnProcessorTripleTrain(HunyuanVideoFlashAttnProcessorTripleEval):
    """Training-time soft mixture of the three experts (hunyuan.py:241-513): every head runs all three experts and the
    outputs are summed with the routing scores.  By default (`differentiable=False`) it is a forward:
    a call that would need gradients raises instead of silently returning a detached result.
    `use_original_attn=True` (the dense teacher, hunyuan.py:312-321) is the dense processor.
    With `differentiable=True` a call in grad mode is the TRAINING forward instead: the same launches behind
    `soft_mixture_attention_autograd`, with gradients for hidden_states, encoder_hidden_states, routing_score and the
    module parameters.
    Both forms run under sequence parallelism (attention/_sp.py `sp_soft_mixture_attention[_autograd]`): the heads are
    resharded once, a rank mixes its own heads, and in grad mode the exchange is differentiable.  A rank then holds the
    gradient of the replicated text rows (and of routing_score) for its own heads only: the training loop sums them over
    the sequence-parallel group, like the parameter gradients.  The dense teacher stays a torch.no_grad() call there."""

    _HAS_BACKWARD = True

    def __call__(self, attn, hidden_states, encoder_hidden_states, attention_mask, image_rotary_emb,
                 use_original_attn: bool = False, routing_score: Optional[torch.Tensor] = None,
                 lowres_group_info: Optional[LowresGroupInfo] = None,
                 flex_attn_mask_func: Optional[SlidingTileDescriptor] = None,
                 window_size: Tuple[int, int, int] = (3, 3, 3), tile_size: Tuple[int, int, int] = (6, 8, 8),
                 latent_shape: Tuple[int, int, int] = (30, 48, 80), fidelity: Optional[list] = None):
        """fidelity: a list that receives this call's `ops.ExpertFidelity` (the heads this process holds: all of them, or this
        rank's under sequence parallelism); None: the launches of today"""
        if use_original_attn:
            return HunyuanVideoFlashAttnProcessor.__call__(self, attn, hidden_states, encoder_hidden_states,
                                                           attention_mask, image_rotary_emb)
        if self._grad_path(sequence_parallel=True):
            self._check_input(hidden_states, lowres_group_info, latent_shape, window_size, tile_size)
            q, k, v, T = self._project(attn, hidden_states, encoder_hidden_states, image_rotary_emb, grad=True)
            assert q.shape[0] == 1, f"Batch size {q.shape[0]} is not supported for {self.__class__.__name__}."
            te = self._text_valid(attention_mask, T, flex_attn_mask_func)
            if SP_STATE.enabled:  # norm + RoPE ran on the local shard (rotary rows shrunk in `_project`); whole heads after the exchange
                from ._sp import sp_soft_mixture_attention_autograd
                buf = sp_soft_mixture_attention_autograd(q, k, v, T, routing_score, model="hunyuan", text_valid=te,
                                                         lowres_group_info=lowres_group_info, window_size=window_size,
                                                         tile_size=tile_size, latent_shape=latent_shape, fidelity=fidelity)
                return self._output(attn, buf, T)
            geom = geometry_for(**_torch_ops.geometry_args(lowres_group_info, window_size, tile_size, latent_shape),
                                device=q.device)
            out = soft_mixture_attention_autograd(q.contiguous(), k.contiguous(), v.contiguous(), routing_score, geom,
                                                  model="hunyuan", text_len=T, text_valid=te, fidelity=fidelity)
            return self._output(attn, out.transpose(1, 2), T)
        if torch.is_grad_enabled() and (hidden_states.requires_grad or routing_score.requires_grad):
            raise NotImplementedError("the soft-mixture forward of this build has no backward: call it under "
                                      "torch.no_grad() (router training is outside the inference hot path)")
        with torch.no_grad():
            self._check_input(hidden_states, lowres_group_info, latent_shape, window_size, tile_size)
            q, k, v, T = self._project(attn, hidden_states, encoder_hidden_states, image_rotary_emb)
            assert q.shape[0] == 1, f"Batch size {q.shape[0]} is not supported for {self.__class__.__name__}."
            te = self._text_valid(attention_mask, T, flex_attn_mask_func)
            if SP_STATE.enabled:
                from ._sp import sp_soft_mixture_attention
                buf = sp_soft_mixture_attention(q, k, v, T, routing_score, model="hunyuan", text_valid=te,
                                                lowres_group_info=lowres_group_info, window_size=window_size,
                                                tile_size=tile_size, latent_shape=latent_shape, fidelity=fidelity)
                return self._output(attn, buf, T)
            buf, out = self._new_out(q)
            if fidelity is not None:  # (a list is no operator argument: the launcher behind vorta::soft_mixture_attention, directly)
                from ..routed import soft_mixture_attention
                geom = geometry_for(**_torch_ops.geometry_args(lowres_group_info, window_size, tile_size, latent_shape),
                                    device=q.device)
                soft_mixture_attention(q, k, v, routing_score, geom, model="hunyuan", text_len=T, text_valid=te, out=out,
                                       fidelity=fidelity)
                return self._output(attn, buf, T)
            torch.ops.vorta.soft_mixture_attention(q, k, v, routing_score, out,
                                                   **_torch_ops.geometry_args(lowres_group_info, window_size, tile_size,
                                                                              latent_shape),
                                                   model="hunyuan", text_len=T, text_valid=te)
            return self._output(attn, buf, T)
