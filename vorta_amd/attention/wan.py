"""Wan-2.1 attention processors (video-only self attention + separate cross attention).

Same classes, call protocol and keyword names as vorta/attention/wan.py.  Only self attention is routed
(modeling_wan.py:215-229); cross attention and `use_original_attn` go through the dense kernel.
"""
from typing import List, Optional, Tuple

import torch

from .. import ops
from .. import torch_ops as _torch_ops  # registers torch.ops.vorta.*: what the processors launch through
from ..routed import (HeadRouting, dense_attention, dense_attention_autograd, geometry_for, qk_norm_rope_autograd,
                      soft_mixture_attention_autograd)
from ..ulysses import SP_STATE, shrink_dim
from ._eval import check_eval_input, launch_routes, refuse_under_sequence_parallel, resolve_routes
from .coreset_select import LowresGroupInfo
from .sliding_tile import SlidingTileDescriptor


def apply_rotary_emb(hidden_states: torch.Tensor, freqs: torch.Tensor) -> torch.Tensor:
    """complex rotation in float64, as the reference does it (wan.py:34-37); before the attention boundary."""
    x = torch.view_as_complex(hidden_states.to(torch.float64).unflatten(3, (-1, 2)))
    return torch.view_as_real(x * freqs).flatten(3, 4).type_as(hidden_states)


_ROPE_CACHE = {}


def _cos_sin(freqs: torch.Tensor):
    """complex frequencies (1,1,S,D/2) -> fp32 (cos, sin) of shape (S,D) with each value repeated for its pair.
    One entry, keyed on the frequency tensor OBJECT (held by the entry: a freed tensor's address is routinely reused
    for the next forward's table, e.g. 480x832 then 832x480 give equal shapes and different contents) and its version:
    the 30-40 blocks of one forward share the tensor (modeling_wan.py:242-262), the next forward builds a new one."""
    hit = _ROPE_CACHE.get("entry")
    if hit is not None and hit[0] is freqs and hit[1] == freqs._version:
        return hit[2]
    f = freqs.reshape(-1, freqs.shape[-1])
    cs = (f.real.float().repeat_interleave(2, dim=1).contiguous(), f.imag.float().repeat_interleave(2, dim=1).contiguous())
    _ROPE_CACHE["entry"] = (freqs, freqs._version, cs)
    return cs


class WanAttnProcessor2_0:
    """Dense attention (wan.py:40-160): self, text cross (Sq != Skv) and the optional I2V image branch.

    `differentiable=True` (off by default): a call in grad mode builds an autograd graph from the output back to
    hidden_states, encoder_hidden_states and the module parameters (`qk_norm_rope_autograd`, `dense_attention_autograd`);
    under torch.no_grad() such a processor takes the inference path and gives its bits."""

    _HAS_BACKWARD = True  # the concrete class can sit in a training graph (the Eval class cannot: hard top-1)

    def __init__(self, differentiable: bool = False):
        ops._C.lib()  # no fallback: fail now if the HIP library is missing
        if differentiable and not type(self)._HAS_BACKWARD:
            raise ValueError(f"{type(self).__name__} routes every head to its top-1 expert, which has no gradient: "
                             "differentiable=True belongs to the dense and the soft-mixture (Train) processors")
        self.differentiable = bool(differentiable)

    def _grad_path(self, sequence_parallel: bool = False) -> bool:
        """build an autograd graph in this call?  `sequence_parallel`: the caller has a differentiable exchange (the soft
        mixture, attention/_sp.py) or needs none (cross attention: replicated keys); the dense self attention has none --
        the teacher runs under torch.no_grad()"""
        if not (self.differentiable and torch.is_grad_enabled()):
            return False
        if SP_STATE.enabled and not sequence_parallel:
            raise NotImplementedError("differentiable=True of the dense attention is not sequence-parallel in this build: "
                                      "only the soft mixture has a differentiable exchange")
        return True

    def _input_proj(self, attn, hidden_states, encoder_hidden_states=None, rotary_emb=None, grad: bool = False):
        """wan.py:64-101: q/k/v projections, RMSNorm across heads (before the head split), RoPE.
        grad=True: the norm + RoPE pass is the out-of-place, differentiable one."""
        enc_img = None
        if attn.add_k_proj is not None:
            enc_img = encoder_hidden_states[:, :257]
            encoder_hidden_states = encoder_hidden_states[:, 257:]
        if encoder_hidden_states is None:
            encoder_hidden_states = hidden_states
        q = attn.to_q(hidden_states)
        k = attn.to_k(encoder_hidden_states)
        v = attn.to_v(encoder_hidden_states)
        H = attn.heads
        rope = shrink_dim(rotary_emb, dim=2) if rotary_emb is not None else None
        from .hunyuan import _fusable_norm
        fuse = (q.shape[0] == 1 and q.shape[-1] == H * 128
                and (rope is None or (rope.shape[-2] == q.shape[1] == k.shape[1]))
                and _fusable_norm(attn.norm_q, q.view(1, q.shape[1], H, 128), H * 128)
                and _fusable_norm(attn.norm_k, k.view(1, k.shape[1], H, 128), H * 128))
        if fuse:
            # RMSNorm over all H*D channels of a token + rotation, one in-place HIP pass per tensor
            cos, sin = _cos_sin(rope) if rope is not None else (None, None)
            q, k, v = (x.unflatten(2, (H, -1)).transpose(1, 2) for x in (q, k, v))
            if grad:
                q = qk_norm_rope_autograd(q, attn.norm_q.weight, float(attn.norm_q.eps), cos, sin, None, True)
                k = qk_norm_rope_autograd(k, attn.norm_k.weight, float(attn.norm_k.eps), cos, sin, None, True)
            else:
                torch.ops.vorta.qk_norm_rope(q[0], attn.norm_q.weight, float(attn.norm_q.eps), cos, sin, -1, True)
                torch.ops.vorta.qk_norm_rope(k[0], attn.norm_k.weight, float(attn.norm_k.eps), cos, sin, -1, True)
        else:
            if attn.norm_q is not None:
                q = attn.norm_q(q)
            if attn.norm_k is not None:
                k = attn.norm_k(k)
            q, k, v = (x.unflatten(2, (H, -1)).transpose(1, 2) for x in (q, k, v))
            if rope is not None:
                q, k = apply_rotary_emb(q, rope), apply_rotary_emb(k, rope)
        return q, k, v, enc_img

    @staticmethod
    def _new_out(q: torch.Tensor):
        B, H, N, D = q.shape
        buf = torch.empty((B, N, H, D), dtype=q.dtype, device=q.device)
        return buf, buf.permute(0, 2, 1, 3)

    def _attn(self, attn, q, k, v, enc_img, is_cross_attn: bool):
        """wan.py:103-149 without SP (the SP branch lives in _sp.py). Returns (B,S,H,D) buffers."""
        buf_img = None
        if enc_img is not None:
            k_img = attn.norm_added_k(attn.add_k_proj(enc_img)).unflatten(2, (attn.heads, -1)).transpose(1, 2)
            v_img = attn.add_v_proj(enc_img).unflatten(2, (attn.heads, -1)).transpose(1, 2)
            buf_img, out_img = self._new_out(q)
            for b in range(q.shape[0]):
                dense_attention(q[b:b + 1], k_img[b:b + 1], v_img[b:b + 1], out=out_img[b:b + 1])
        buf, out = self._new_out(q)
        for b in range(q.shape[0]):
            dense_attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], out=out[b:b + 1])
        return buf, buf_img

    @staticmethod
    def _attn_grad(attn, q, k, v, enc_img):
        """`_attn` behind autograd (dense_attention_autograd folds a batch into the head axis)"""
        buf_img = None
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        if enc_img is not None:
            k_img = attn.norm_added_k(attn.add_k_proj(enc_img)).unflatten(2, (attn.heads, -1)).transpose(1, 2)
            v_img = attn.add_v_proj(enc_img).unflatten(2, (attn.heads, -1)).transpose(1, 2)
            buf_img = dense_attention_autograd(q, k_img.contiguous(), v_img.contiguous()).transpose(1, 2)
        return dense_attention_autograd(q, k, v).transpose(1, 2), buf_img

    @staticmethod
    def _output_proj(attn, buf, buf_img=None):
        hidden = buf.flatten(2, 3)
        if buf_img is not None:
            hidden = hidden + buf_img.flatten(2, 3)
        return attn.to_out[1](attn.to_out[0](hidden))

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, rotary_emb=None):
        """Cross attention (`encoder_hidden_states` given) in grad mode under sequence parallelism is LOCAL: a rank holds
        all heads of its query shard and every text / image key (`_sp.sp_wan_dense`), so the grad path below runs on the
        shard as it is and no collective is issued, forward or backward.  A rank ends with its own rows of
        d hidden_states, whole; with a PARTIAL gradient of encoder_hidden_states and of to_k / to_v / add_k_proj /
        add_v_proj / norm_k / norm_added_k (the keys are replicated, the queries that read them are not), which sum over
        the ranks to the single-process gradient; and with the gradient of to_q / norm_q / to_out from its own rows,
        which sums over the ranks like that of any parameter applied to a sequence shard.  Dense SELF attention in grad
        mode under sequence parallelism keeps raising: it has no differentiable exchange."""
        # the default: no autograd graph, whatever the inputs ask for
        if not self._grad_path(sequence_parallel=encoder_hidden_states is not None):
            return self._call_no_grad(attn, hidden_states, encoder_hidden_states, attention_mask, rotary_emb)
        if attention_mask is not None:
            raise NotImplementedError("attention_mask is always None on this path (wan.py:141)")
        q, k, v, enc_img = self._input_proj(attn, hidden_states, encoder_hidden_states, rotary_emb, grad=True)
        return self._output_proj(attn, *self._attn_grad(attn, q, k, v, enc_img))

    @torch.no_grad()  # forward only
    def _call_no_grad(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, rotary_emb=None):
        if attention_mask is not None:
            raise NotImplementedError("attention_mask is always None on this path (wan.py:141)")
        is_cross = encoder_hidden_states is not None
        q, k, v, enc_img = self._input_proj(attn, hidden_states, encoder_hidden_states, rotary_emb)
        if SP_STATE.enabled:
            from ._sp import sp_wan_dense
            return self._output_proj(attn, *sp_wan_dense(self, attn, q, k, v, enc_img, is_cross))
        return self._output_proj(attn, *self._attn(attn, q, k, v, enc_img, is_cross))


class WanAttnProcessorTripleEval(WanAttnProcessor2_0):
    """Inference-time routed self attention (wan.py:303-437)."""

    _HAS_BACKWARD = False

    def __init__(self, check_input: bool = False, differentiable: bool = False):
        super().__init__(differentiable)
        self.check_input = check_input

    def _check_input(self, hidden_states, lowres_group_info, latent_shape, window_size, tile_size):
        """wan.py:168-193: attention/_eval.py `check_eval_input`"""
        if not self.check_input:
            return
        check_eval_input(hidden_states, lowres_group_info, latent_shape, window_size, tile_size)

    @torch.no_grad()
    def __call__(self, attn, hidden_states, encoder_hidden_states, attention_mask, rotary_emb,
                 tau_sparse: float, routing_score: torch.Tensor,
                 lowres_group_info: Optional[LowresGroupInfo] = None,
                 flex_attn_mask_func: Optional[SlidingTileDescriptor] = None,
                 window_size: Tuple[int, int, int] = (3, 3, 3), tile_size: Tuple[int, int, int] = (6, 8, 8),
                 latent_shape: Tuple[int, int, int] = (20, 30, 52), use_original_attn: bool = False,
                 head_routing: Optional[HeadRouting] = None, experts_host: Optional[List[int]] = None,
                 fidelity: Optional[list] = None, fidelity_rows=None, fidelity_heads: str = "sparse",
                 expert_fidelity: Optional[list] = None, route_rule=None, route_sink: Optional[list] = None,
                 tier_routing: Optional[dict] = None, repair_above: Optional[float] = None,
                 repair_sink: Optional[list] = None):
        """Keyword names as wan.py:308-328; `head_routing` / `experts_host`: see the Hunyuan processor.
        fidelity: a list that receives one `ops.SampledFidelity` PER BATCH ITEM of this call, in item order (the routed output
        as run against dense attention on sampled rows, routed.routed_attention); cross attention and the dense teacher file
        nothing; None: the launches of today.  expert_fidelity: likewise one `ops.ExpertFidelity` per batch item
        (routed.sampled_expert_fidelity on the same `fidelity_rows`); refused by name under sequence parallelism.
        route_rule / route_sink, `covers_precision`, `tier_routing`, repair_above / repair_sink: see the Hunyuan processor, and
        attention/_eval.py for a batch: every item is routed by ITEM 0's measurement (the reference's convention for scores,
        quoted below; one sink entry per call), item 0 alone launches on the operands the measurement prepared, and item 0
        alone is verified and repaired (one record per call) -- every other item launches the repaired tables."""
        if encoder_hidden_states is not None or use_original_attn:
            return WanAttnProcessor2_0.__call__(self, attn, hidden_states, encoder_hidden_states, attention_mask,
                                                rotary_emb)
        self._check_input(hidden_states, lowres_group_info, latent_shape, window_size, tile_size)
        q, k, v, _ = self._input_proj(attn, hidden_states, None, rotary_emb)
        B = q.shape[0]
        # the reference routes EVERY batch item by item 0's scores (wan.py:388-416: `routing_score[0].topk(1)`); the kernels
        # take one item per launch, so a batch is a loop over its items with the same routes (the scripts run B = 1:
        # pipeline_wan.py:322-344 does CFG as two forwards)
        if SP_STATE.enabled:
            refuse_under_sequence_parallel(expert_fidelity, route_rule, tier_routing, repair_above)
            from ._sp import sp_attention
            bufs = [sp_attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], 0, routing_score, tau_sparse, model="wan",
                                 lowres_group_info=lowres_group_info, window_size=window_size, tile_size=tile_size,
                                 latent_shape=latent_shape, experts_host=experts_host, fidelity=fidelity,
                                 fidelity_rows=fidelity_rows, fidelity_heads=fidelity_heads) for b in range(B)]
            return self._output_proj(attn, bufs[0] if B == 1 else torch.cat(bufs, dim=0))
        geometry = _torch_ops.geometry_args(lowres_group_info, window_size, tile_size, latent_shape)
        routes = resolve_routes(q, k, v, geometry, model="wan", routing_score=routing_score, tau_sparse=tau_sparse,
                                head_routing=head_routing, route_rule=route_rule, route_sink=route_sink, tier_routing=tier_routing)
        buf, out = self._new_out(q)
        launch_routes(q, k, v, out, routes, geometry, model="wan", fidelity=fidelity, fidelity_rows=fidelity_rows,
                      fidelity_heads=fidelity_heads, expert_fidelity=expert_fidelity, repair_above=repair_above,
                      repair_sink=repair_sink)
        return self._output_proj(attn, buf)


class WanAttnProcessorTripleTrain(WanAttnProcessorTripleEval):
    """Soft-mixture training forward (wan.py:163-300); the dense teacher (`use_original_attn=True`)
    and cross attention are the dense processor.  By default (`differentiable=False`) a call that would need gradients
    raises.  With `differentiable=True` a call in grad mode is the TRAINING forward instead: the same launches behind
    `soft_mixture_attention_autograd`, with gradients for hidden_states, routing_score and the module parameters.
    Both forms run under sequence parallelism (attention/_sp.py `sp_soft_mixture_attention[_autograd]`); in grad mode a
    rank holds d routing_score for its own heads only (summed over the group by the training loop, like the parameter
    gradients).  The dense teacher stays a torch.no_grad() call there."""

    _HAS_BACKWARD = True

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, rotary_emb=None,
                 use_original_attn: bool = False, routing_score: Optional[torch.Tensor] = None,
                 lowres_group_info: Optional[LowresGroupInfo] = None,
                 flex_attn_mask_func: Optional[SlidingTileDescriptor] = None,
                 window_size: Tuple[int, int, int] = (3, 3, 3), tile_size: Tuple[int, int, int] = (6, 8, 8),
                 latent_shape: Tuple[int, int, int] = (20, 30, 52), fidelity: Optional[list] = None):
        """fidelity: a list that receives this call's `ops.ExpertFidelity` (the heads this process holds: all of them, or this
        rank's under sequence parallelism); None: the launches of today"""
        if encoder_hidden_states is not None or use_original_attn:
            return WanAttnProcessor2_0.__call__(self, attn, hidden_states, encoder_hidden_states, attention_mask,
                                                rotary_emb)
        if self._grad_path(sequence_parallel=True):
            self._check_input(hidden_states, lowres_group_info, latent_shape, window_size, tile_size)
            q, k, v, _ = self._input_proj(attn, hidden_states, None, rotary_emb, grad=True)
            assert q.shape[0] == 1, "the soft mixture runs one batch item per call"
            if SP_STATE.enabled:  # norm + RoPE ran on the local shard (rotary rows shrunk in `_input_proj`)
                from ._sp import sp_soft_mixture_attention_autograd
                buf = sp_soft_mixture_attention_autograd(q, k, v, 0, routing_score, model="wan",
                                                         lowres_group_info=lowres_group_info, window_size=window_size,
                                                         tile_size=tile_size, latent_shape=latent_shape, fidelity=fidelity)
                return self._output_proj(attn, buf)
            geom = geometry_for(**_torch_ops.geometry_args(lowres_group_info, window_size, tile_size, latent_shape),
                                device=q.device)
            out = soft_mixture_attention_autograd(q.contiguous(), k.contiguous(), v.contiguous(), routing_score, geom,
                                                  model="wan", fidelity=fidelity)
            return self._output_proj(attn, out.transpose(1, 2))
        if torch.is_grad_enabled() and (hidden_states.requires_grad or routing_score.requires_grad):
            raise NotImplementedError("the soft-mixture forward of this build has no backward: call it under "
                                      "torch.no_grad() (router training is outside the inference hot path)")
        with torch.no_grad():
            self._check_input(hidden_states, lowres_group_info, latent_shape, window_size, tile_size)
            q, k, v, _ = self._input_proj(attn, hidden_states, None, rotary_emb)
            assert q.shape[0] == 1, "the soft mixture runs one batch item per call"
            if SP_STATE.enabled:
                from ._sp import sp_soft_mixture_attention
                buf = sp_soft_mixture_attention(q, k, v, 0, routing_score, model="wan", lowres_group_info=lowres_group_info,
                                                window_size=window_size, tile_size=tile_size, latent_shape=latent_shape,
                                                fidelity=fidelity)
                return self._output_proj(attn, buf)
            buf, out = self._new_out(q)
            if fidelity is not None:  # (a list is no operator argument: the launcher behind vorta::soft_mixture_attention, directly)
                from ..routed import soft_mixture_attention
                geom = geometry_for(**_torch_ops.geometry_args(lowres_group_info, window_size, tile_size, latent_shape),
                                    device=q.device)
                soft_mixture_attention(q, k, v, routing_score, geom, model="wan", out=out, fidelity=fidelity)
                return self._output_proj(attn, buf)
            torch.ops.vorta.soft_mixture_attention(q, k, v, routing_score, out,
                                                   **_torch_ops.geometry_args(lowres_group_info, window_size, tile_size,
                                                                              latent_shape), model="wan")
            return self._output_proj(attn, buf)
