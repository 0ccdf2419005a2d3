"""`torch.ops.vorta.*`: the launchers of vorta_amd/ops.py registered as PyTorch custom ops.

The C ABI (include/vorta_hip.h) is the boundary; ops.py binds it with ctypes.  This module puts the same launchers
behind `torch.library.custom_op`, so code that is traced (`torch.compile`, export) sees them as opaque, stream-correct
operators with declared mutations and shape functions instead of Python it cannot follow (BASELINE.json north star:
"Python host code calls into hand-written HIP kernels through PyTorch-ROCm custom ops (thin C-ABI ...)").  The
attention processors of vorta_amd/attention call THESE operators (`vorta::routed_attention`, `vorta::attn_fwd`,
`vorta::qk_norm_rope`, `vorta::route_scores`, `vorta::soft_mixture_attention`; the route plan of patch/_engine.py
`vorta::route_plan_`): a processor `__call__` traces under `torch.compile(fullgraph=True)` with no graph break, and the
eager path runs the very same launchers behind one dispatcher hop per operator.

Registered (tensors are (H,S,D) views as in ops.py; optional tensors may be None):
    vorta::attn_fwd(q,k,v,out, n_q,n_kv, ...)         -> ()    mutates out        vorta_attn_fwd
    vorta::coreset_select(x, latent, group, n_keep, ...) -> (keep_rows, drop_rows)  vorta_coreset_select
    vorta::sta_build_tables(like, latent, tile, window, t_eff, row_map) -> (q_rows, kv_rows)
    vorta::route_scores(scores, tau)                  -> (expert_of_head, head_lists, head_counts)
    vorta::route_fidelity(sq_ref, sq_err, max_rel_error, max_flops_share, work)
                                                      -> (expert_of_head, head_lists, head_counts, flops_share)   vorta_route_fidelity
    vorta::route_fidelity_tiers(sq_ref, sq_err, tiers, max_rel_error, work, tier_cost)
                                                      -> (expert_of_head, tier_of_head, head_lists, head_counts, cost_share)   vorta_route_fidelity_tiers
    vorta::route_budget_tiers(sq_ref, sq_err, tiers, max_cost_share, work, tier_cost)
                                                      -> (expert_of_head, tier_of_head, head_lists, head_counts, level, cost_share)   vorta_route_budget_tiers
    vorta::route_repair(sq_ref, sq_err, expert_of_head, tier_of_head, head_lists, head_counts, exact_tier, repair_above)
                                                      -> (repair_list, repair_count, state_of_head, rel)   mutates the four tables   vorta_route_repair
    vorta::router_route(temb, weight, bias, heads, tau) -> (scores, expert_of_head, head_lists, head_counts)
    vorta::qk_norm_rope(x, weight, eps, cos, sin, rope_tokens, across_heads) -> () mutates x
    vorta::mix_experts(x0,x1,x2, scores, out)         -> ()    mutates out
    vorta::routed_attention(q,k,v,out, head_lists, head_counts, counts_host, latent, tile, window, group, rate, model, ...)
                                                      -> ()    mutates out        the per-layer routed op (routed.py)
    vorta::soft_mixture_attention(q,k,v, scores, out, latent, ...) -> () mutates out   the training-time forward
    vorta::route_plan_(temb, weight, bias, heads, tau, n_experts, scores, expert, lists, counts) -> () mutates the four
    vorta::soft_mixture_attention_grad(q,k,v, scores, latent, ...) -> out   functional, differentiable (register_autograd);
    vorta::soft_mixture_attention_bwd(q,k,v, scores, d_out, latent, ...) -> (dq, dk, dv, dscores)   its autograd formula
    vorta::qk_norm_rope_grad(x, weight, eps, cos, sin, rope_tokens, across_heads) -> y   out of place, differentiable;
    vorta::qk_norm_rope_bwd(x, g, weight, eps, cos, sin, ...) -> (dx, dweight)   its autograd formula (vorta_qk_norm_rope_bwd)
    vorta::expert_fidelity(x0,x1,x2, mixed)           -> (sq_ref, max_ref, sq_err, max_err, range_ref)   vorta_expert_fidelity
    vorta::sampled_fidelity(ref, out, rows, head_list, n_heads, n_heads_dev, row_errors)
                                                      -> (sq_ref, max_ref, sq_err, max_err, range_ref, row_sq_err)   vorta_sampled_fidelity
"""
from typing import List, Optional, Tuple

import torch

from . import ops


@torch.library.custom_op("vorta::attn_fwd", mutates_args=("out",), device_types="cuda")
def attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, n_q: int, n_kv: int,
             head_list: Optional[torch.Tensor] = None, n_heads: int = -1, n_heads_dev: Optional[torch.Tensor] = None,
             q_group_len: int = 0, q_row_offset: int = 0, q_valid: int = -1, q_rows: Optional[torch.Tensor] = None,
             kv_row_offset: int = 0, kv_rows: Optional[torch.Tensor] = None, kv_rows_stride_g: int = 0,
             dup_rows: Optional[torch.Tensor] = None, n_dup_pos: int = 0, scale: float = 0.0, block_rows: int = 0,
             n_splits: int = 1, n_kv_dev: Optional[torch.Tensor] = None, q_valid_dev: Optional[torch.Tensor] = None,
             variant: int = 0) -> None:
    ops.attn_fwd(q, k, v, out, n_q=n_q, n_kv=n_kv, head_list=head_list, n_heads=None if n_heads < 0 else n_heads,
                 n_heads_dev=n_heads_dev, q_group_len=q_group_len, q_row_offset=q_row_offset,
                 q_valid=None if q_valid < 0 else q_valid, q_rows=q_rows, kv_row_offset=kv_row_offset, kv_rows=kv_rows,
                 kv_rows_stride_g=kv_rows_stride_g, dup_rows=dup_rows, n_dup_pos=n_dup_pos,
                 scale=None if scale <= 0.0 else scale, block_rows=block_rows, n_splits=n_splits, n_kv_dev=n_kv_dev,
                 q_valid_dev=q_valid_dev, variant=variant)


@attn_fwd.register_fake
def _(q, k, v, out, n_q, n_kv, head_list=None, n_heads=-1, n_heads_dev=None, q_group_len=0, q_row_offset=0, q_valid=-1,
      q_rows=None, kv_row_offset=0, kv_rows=None, kv_rows_stride_g=0, dup_rows=None, n_dup_pos=0, scale=0.0,
      block_rows=0, n_splits=1, n_kv_dev=None, q_valid_dev=None, variant=0) -> None:
    return None


def _coreset_shapes(x, latent, group, n_keep, head_list, n_heads, n_tail):
    slots = n_heads if n_heads >= 0 else (head_list.numel() if head_list is not None else x.shape[0])
    g = group[0] * group[1] * group[2]
    G = (latent[0] // group[0]) * (latent[1] // group[1]) * (latent[2] // group[2])
    return (slots, G * (1 + n_keep) + n_tail), (slots, G, g - 1 - n_keep)


@torch.library.custom_op("vorta::coreset_select", mutates_args=(), device_types="cuda")
def coreset_select(x: torch.Tensor, latent: List[int], group: List[int], n_keep: int,
                   head_list: Optional[torch.Tensor] = None, n_heads: int = -1,
                   n_heads_dev: Optional[torch.Tensor] = None, tail_first: int = 0, n_tail: int = 0,
                   row_map: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    keep, drop = ops.coreset_select(x, latent, group, n_keep, head_list=head_list,
                                    n_heads=None if n_heads < 0 else n_heads, n_heads_dev=n_heads_dev,
                                    tail_first=tail_first, n_tail=n_tail, row_map=row_map)
    return keep, drop


@coreset_select.register_fake
def _(x, latent, group, n_keep, head_list=None, n_heads=-1, n_heads_dev=None, tail_first=0, n_tail=0, row_map=None):
    ks, ds = _coreset_shapes(x, latent, group, n_keep, head_list, n_heads, n_tail)
    return x.new_empty(ks, dtype=torch.int32), x.new_empty(ds, dtype=torch.int32)


@torch.library.custom_op("vorta::sta_build_tables", mutates_args=(), device_types="cuda")
def sta_build_tables(like: torch.Tensor, latent: List[int], tile: List[int], window: List[int], t_eff: int = 0,
                     row_map: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`like` only names the device (custom ops take no device argument)."""
    q_rows, kv_rows = ops.sta_build_tables(latent, tile, window, t_eff, like.device, row_map=row_map)
    return q_rows, kv_rows


@sta_build_tables.register_fake
def _(like, latent, tile, window, t_eff=0, row_map=None):
    n_tiles, _, n_kv = ops.sta_table_sizes(latent, tile, window, t_eff)  # host-only geometry query
    S = latent[0] * latent[1] * latent[2]
    return like.new_empty((S,), dtype=torch.int32), like.new_empty((n_tiles, n_kv), dtype=torch.int32)


@torch.library.custom_op("vorta::route_scores", mutates_args=(), device_types="cuda")
def route_scores(scores: torch.Tensor, tau: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.route_scores(scores, tau)


@route_scores.register_fake
def _(scores, tau):
    _, H, E = scores.shape
    i32 = dict(dtype=torch.int32)
    return scores.new_empty((H,), **i32), scores.new_empty((E, H), **i32), scores.new_empty((E,), **i32)


@torch.library.custom_op("vorta::route_fidelity", mutates_args=(), device_types="cuda")
def route_fidelity(sq_ref: torch.Tensor, sq_err: torch.Tensor, max_rel_error: Optional[float] = None,
                   max_flops_share: Optional[float] = None, work: Optional[List[float]] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """ops.route_fidelity on the statistics of one layer, sq_ref (H,) and sq_err (H,3): int32 (H,), (3,H), (3,) and the
    routed layer's share of the dense FLOPs, float32 (1,); exactly one of `max_rel_error` and `max_flops_share`"""
    return ops.route_fidelity(ops.ExpertFidelity(sq_ref, sq_ref, sq_err, sq_err), max_rel_error=max_rel_error,
                              max_flops_share=max_flops_share, work=work, flops_share=True)


@route_fidelity.register_fake
def _(sq_ref, sq_err, max_rel_error=None, max_flops_share=None, work=None):
    H = sq_ref.shape[0]
    i32 = dict(dtype=torch.int32)
    return (sq_ref.new_empty((H,), **i32), sq_ref.new_empty((3, H), **i32), sq_ref.new_empty((3,), **i32),
            sq_ref.new_empty((1,), dtype=torch.float32))


@torch.library.custom_op("vorta::route_fidelity_tiers", mutates_args=(), device_types="cuda")
def route_fidelity_tiers(sq_ref: torch.Tensor, sq_err: torch.Tensor, tiers: List[int], max_rel_error: float,
                         work: Optional[List[float]] = None, tier_cost: Optional[List[float]] = None
                         ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """ops.route_fidelity_tiers on the statistics of one layer: sq_ref (H,), sq_err (n_tiers,H,3), `tiers` the global tier ids
    of sq_err's leading axis in the caller's order, `tier_cost` their costs in that order (None: ops.DEFAULT_TIER_COST):
    int32 (H,), (H,), (n_tiers,3,H), (n_tiers,3) and the routed layer's cost share, float32 (1,)"""
    if sq_err.dim() != 3 or sq_err.shape[0] != len(tiers) or (tier_cost is not None and len(tier_cost) != len(tiers)):
        raise ValueError("route_fidelity_tiers: sq_err (n_tiers, H, 3) with one tier id, and one cost where given, per tier")
    fids = {t: ops.ExpertFidelity(sq_ref, sq_ref, sq_err[i], sq_err[i]) for i, t in enumerate(tiers)}
    if len(fids) != len(tiers):
        raise ValueError(f"route_fidelity_tiers: distinct tiers, got {list(tiers)}")
    cost = None if tier_cost is None else dict(zip(tiers, tier_cost))
    return ops.route_fidelity_tiers(fids, max_rel_error=max_rel_error, work=work, tier_cost=cost, cost_share=True)


@route_fidelity_tiers.register_fake
def _(sq_ref, sq_err, tiers, max_rel_error, work=None, tier_cost=None):
    H, T = sq_ref.shape[0], len(tiers)
    i32 = dict(dtype=torch.int32)
    return (sq_ref.new_empty((H,), **i32), sq_ref.new_empty((H,), **i32), sq_ref.new_empty((T, 3, H), **i32),
            sq_ref.new_empty((T, 3), **i32), sq_ref.new_empty((1,), dtype=torch.float32))


@torch.library.custom_op("vorta::route_budget_tiers", mutates_args=(), device_types="cuda")
def route_budget_tiers(sq_ref: torch.Tensor, sq_err: torch.Tensor, tiers: List[int], max_cost_share: float,
                       work: Optional[List[float]] = None, tier_cost: Optional[List[float]] = None
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """ops.route_budget_tiers on the statistics of one layer: the arguments of `route_fidelity_tiers` with the share of the
    all-dense cost in the bound's place: int32 (H,), (H,), (n_tiers,3,H), (n_tiers,3), the level float32 (1,) and the routed
    layer's cost share, float32 (1,)"""
    if sq_err.dim() != 3 or sq_err.shape[0] != len(tiers) or (tier_cost is not None and len(tier_cost) != len(tiers)):
        raise ValueError("route_budget_tiers: sq_err (n_tiers, H, 3) with one tier id, and one cost where given, per tier")
    fids = {t: ops.ExpertFidelity(sq_ref, sq_ref, sq_err[i], sq_err[i]) for i, t in enumerate(tiers)}
    if len(fids) != len(tiers):
        raise ValueError(f"route_budget_tiers: distinct tiers, got {list(tiers)}")
    cost = None if tier_cost is None else dict(zip(tiers, tier_cost))
    return ops.route_budget_tiers(fids, max_cost_share=max_cost_share, work=work, tier_cost=cost, cost_share=True)


@route_budget_tiers.register_fake
def _(sq_ref, sq_err, tiers, max_cost_share, work=None, tier_cost=None):
    H, T = sq_ref.shape[0], len(tiers)
    i32 = dict(dtype=torch.int32)
    return (sq_ref.new_empty((H,), **i32), sq_ref.new_empty((H,), **i32), sq_ref.new_empty((T, 3, H), **i32),
            sq_ref.new_empty((T, 3), **i32), sq_ref.new_empty((1,), dtype=torch.float32),
            sq_ref.new_empty((1,), dtype=torch.float32))


@torch.library.custom_op("vorta::route_repair", mutates_args=("expert_of_head", "tier_of_head", "head_lists", "head_counts"),
                         device_types="cuda")
def route_repair(sq_ref: torch.Tensor, sq_err: torch.Tensor, expert_of_head: torch.Tensor,
                 tier_of_head: Optional[torch.Tensor], head_lists: torch.Tensor, head_counts: torch.Tensor, exact_tier: int,
                 repair_above: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """ops.route_repair on the record of one layer, sq_ref (H,) and sq_err (H,): the int32 route tables expert_of_head (H,),
    tier_of_head (H,) or None, head_lists (n_tiers,3,H) and head_counts (n_tiers,3) are updated in place; returns the heads
    repaired by this call int32 (H,), their count int32 (1,), the state int32 (H,) and rel float32 (H,)"""
    return ops.route_repair(sq_ref, sq_err, expert_of_head, tier_of_head, head_lists, head_counts, exact_tier=exact_tier,
                            repair_above=repair_above)


@route_repair.register_fake
def _(sq_ref, sq_err, expert_of_head, tier_of_head, head_lists, head_counts, exact_tier, repair_above):
    H = sq_ref.shape[0]
    i32 = dict(dtype=torch.int32)
    return (sq_ref.new_empty((H,), **i32), sq_ref.new_empty((1,), **i32), sq_ref.new_empty((H,), **i32),
            sq_ref.new_empty((H,), dtype=torch.float32))


@torch.library.custom_op("vorta::router_route", mutates_args=(), device_types="cuda")
def router_route(temb: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, heads: int, tau: float,
                 n_experts: int = 3) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    return ops.router_route(temb, weight, bias, heads, tau, n_experts)


@router_route.register_fake
def _(temb, weight, bias, heads, tau, n_experts=3):
    i32 = dict(dtype=torch.int32)
    return (temb.new_empty((temb.shape[0], heads, n_experts)), temb.new_empty((heads,), **i32),
            temb.new_empty((n_experts, heads), **i32), temb.new_empty((n_experts,), **i32))


@torch.library.custom_op("vorta::qk_norm_rope", mutates_args=("x",), device_types="cuda")
def qk_norm_rope(x: torch.Tensor, weight: Optional[torch.Tensor], eps: float, cos: Optional[torch.Tensor] = None,
                 sin: Optional[torch.Tensor] = None, rope_tokens: int = 0, across_heads: bool = False) -> None:
    """rope_tokens < 0: every token the cos / sin tables cover (ops.qk_norm_rope's default)"""
    ops.qk_norm_rope(x, weight, eps, cos=cos, sin=sin, rope_tokens=None if rope_tokens < 0 else rope_tokens,
                     across_heads=across_heads)


@qk_norm_rope.register_fake
def _(x, weight, eps, cos=None, sin=None, rope_tokens=0, across_heads=False) -> None:
    return None


@torch.library.custom_op("vorta::mix_experts", mutates_args=("out",), device_types="cuda")
def mix_experts(x0: torch.Tensor, x1: torch.Tensor, x2: torch.Tensor, scores: torch.Tensor, out: torch.Tensor) -> None:
    ops.mix_experts([x0, x1, x2], scores, out)


@mix_experts.register_fake
def _(x0, x1, x2, scores, out) -> None:
    return None


@torch.library.custom_op("vorta::expert_fidelity", mutates_args=(), device_types="cuda")
def expert_fidelity(x0: torch.Tensor, x1: torch.Tensor, x2: torch.Tensor, mixed: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """ops.expert_fidelity on (H,N,D) views: float32 (H,), (H,), (H,3), (H,3), (H,) -- the fields of ops.ExpertFidelity but `n`
    (= N * D, which a caller knows from the shapes)"""
    f = ops.expert_fidelity([x0, x1, x2], mixed)
    return f.sq_ref, f.max_ref, f.sq_err, f.max_err, f.range_ref


@expert_fidelity.register_fake
def _(x0, x1, x2, mixed=None):
    H = x0.shape[0]
    f32 = dict(dtype=torch.float32)
    return (x0.new_empty((H,), **f32), x0.new_empty((H,), **f32), x0.new_empty((H, 3), **f32), x0.new_empty((H, 3), **f32),
            x0.new_empty((H,), **f32))


@torch.library.custom_op("vorta::sampled_fidelity", mutates_args=(), device_types="cuda")
def sampled_fidelity(ref: torch.Tensor, out: torch.Tensor, rows: torch.Tensor, head_list: Optional[torch.Tensor] = None,
                     n_heads: int = -1, n_heads_dev: Optional[torch.Tensor] = None, row_errors: bool = False
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """ops.sampled_fidelity on ref (H,n,D), out (H,N,D) and rows (n,): float32 (H,) x 5 and (H,n) -- the tensor fields of
    ops.SampledFidelity (row_sq_err is (H,0) without `row_errors`); heads the lists do not name hold NaN.  A device contract,
    checked nowhere (a check would be a host read): every value of `rows` lies in [0, N) and every listed head in [0, H); a
    value outside reads, and a head outside also writes, out of bounds"""
    f = ops.sampled_fidelity(ref, out, rows, head_list, None if n_heads < 0 else n_heads, n_heads_dev, row_errors)
    rows_err = f.row_sq_err if f.row_sq_err is not None else f.sq_ref.new_empty((ref.shape[0], 0))
    return f.sq_ref, f.max_ref, f.sq_err, f.max_err, f.range_ref, rows_err


@sampled_fidelity.register_fake
def _(ref, out, rows, head_list=None, n_heads=-1, n_heads_dev=None, row_errors=False):
    H, n = ref.shape[0], ref.shape[1]
    f32 = dict(dtype=torch.float32)
    return tuple(ref.new_empty((H,), **f32) for _ in range(5)) + (ref.new_empty((H, n if row_errors else 0), **f32),)


@torch.library.custom_op("vorta::routed_attention", mutates_args=("out",), device_types="cuda")
def routed_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, head_lists: torch.Tensor,
                     head_counts: Optional[torch.Tensor], counts_host: Optional[List[int]], latent: List[int],
                     tile: List[int], window: List[int], group: List[int], rate: float, model: str, text_len: int = 0,
                     text_valid: int = 0, scale: float = 0.0, precision: str = "",
                     row_map: Optional[torch.Tensor] = None) -> None:
    """The routed sparse-attention op of one layer (vorta_amd/routed.py: hunyuan.py:556-605 / wan.py:351-383): q,k,v,out
    (1,H,N,D) views; head_lists (3,H) int32 + head_counts (3,) int32 on the device (the route plan's / vorta::route_scores'
    output: no host read) or `counts_host` = the three counts known on the host; the geometry by value (its tables are
    cached per process, routed.geometry_for).  precision "" = the process default (set_attention_precision)."""
    from . import routed
    geom = routed.geometry_for(latent, tile, window, group, rate, q.device, row_map=row_map)
    routing = routed.HeadRouting(head_lists, list(counts_host) if counts_host is not None else None, head_counts)
    routed.routed_attention(q, k, v, routing, geom, model=model, text_len=text_len, text_valid=text_valid, out=out,
                            scale=None if scale <= 0.0 else scale, fp8=routed.precision_of(precision or None))


@routed_attention.register_fake
def _(q, k, v, out, head_lists, head_counts, counts_host, latent, tile, window, group, rate, model, text_len=0,
      text_valid=0, scale=0.0, precision="", row_map=None) -> None:
    return None


@torch.library.custom_op("vorta::soft_mixture_attention", mutates_args=("out",), device_types="cuda")
def soft_mixture_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, routing_score: torch.Tensor, out: torch.Tensor,
                           latent: List[int], tile: List[int], window: List[int], group: List[int], rate: float, model: str,
                           text_len: int = 0, text_valid: int = 0, scale: float = 0.0) -> None:
    """hunyuan.py:375-408,509-513 / wan.py:226-241,296-300, forward only (routed.soft_mixture_attention)"""
    from . import routed
    geom = routed.geometry_for(latent, tile, window, group, rate, q.device)
    routed.soft_mixture_attention(q, k, v, routing_score, geom, model=model, text_len=text_len, text_valid=text_valid,
                                  out=out, scale=None if scale <= 0.0 else scale)


@soft_mixture_attention.register_fake
def _(q, k, v, routing_score, out, latent, tile, window, group, rate, model, text_len=0, text_valid=0, scale=0.0) -> None:
    return None


@torch.library.custom_op("vorta::soft_mixture_attention_grad", mutates_args=(), device_types="cuda")
def soft_mixture_attention_grad(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, routing_score: torch.Tensor,
                                latent: List[int], tile: List[int], window: List[int], group: List[int], rate: float,
                                model: str, text_len: int = 0, text_valid: int = 0, scale: float = 0.0) -> torch.Tensor:
    """The differentiable soft mixture (functional: returns `out`; the mutating vorta::soft_mixture_attention has no
    gradient).  Same launches and bits as routed.soft_mixture_attention; its autograd formula is
    vorta::soft_mixture_attention_bwd."""
    from . import routed
    geom = routed.geometry_for(latent, tile, window, group, rate, q.device)
    return routed.soft_mixture_attention(q, k, v, routing_score, geom, model=model, text_len=text_len, text_valid=text_valid,
                                         scale=None if scale <= 0.0 else scale)


@soft_mixture_attention_grad.register_fake
def _(q, k, v, routing_score, latent, tile, window, group, rate, model, text_len=0, text_valid=0, scale=0.0):
    return torch.empty_like(q)


@torch.library.custom_op("vorta::soft_mixture_attention_bwd", mutates_args=(), device_types="cuda")
def soft_mixture_attention_bwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, routing_score: torch.Tensor,
                               d_out: torch.Tensor, latent: List[int], tile: List[int], window: List[int], group: List[int],
                               rate: float, model: str, text_len: int = 0, text_valid: int = 0,
                               scale: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dq, dk, dv, dscores) of vorta::soft_mixture_attention_grad.  A traced operator keeps no Python state, so the three
    expert outputs and the launch tables are recomputed here (one more forward, deterministic: the same bits and the same
    tables the forward produced) and then differentiated as routed.soft_mixture_attention_autograd does."""
    from . import routed
    geom = routed.geometry_for(latent, tile, window, group, rate, q.device)
    with torch.enable_grad():
        leaves = [x.detach().requires_grad_(True) for x in (q, k, v, routing_score)]
        out = routed.soft_mixture_attention_autograd(*leaves, geom, model=model, text_len=text_len, text_valid=text_valid,
                                                     scale=None if scale <= 0.0 else scale)
        dq, dk, dv, dsc = torch.autograd.grad(out, leaves, d_out)
    return dq, dk, dv, dsc


@soft_mixture_attention_bwd.register_fake
def _(q, k, v, routing_score, d_out, latent, tile, window, group, rate, model, text_len=0, text_valid=0, scale=0.0):
    return torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.empty_like(routing_score)


def _soft_mixture_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:4])
    ctx.rest = inputs[4:]


def _soft_mixture_backward(ctx, d_out):
    q, k, v, sc = ctx.saved_tensors
    grads = torch.ops.vorta.soft_mixture_attention_bwd(q, k, v, sc, d_out.contiguous(), *ctx.rest)
    return (*grads,) + (None,) * len(ctx.rest)


torch.library.register_autograd("vorta::soft_mixture_attention_grad", _soft_mixture_backward,
                                setup_context=_soft_mixture_setup)


@torch.library.custom_op("vorta::qk_norm_rope_grad", mutates_args=(), device_types="cuda")
def qk_norm_rope_grad(x: torch.Tensor, weight: Optional[torch.Tensor], eps: float, cos: Optional[torch.Tensor] = None,
                      sin: Optional[torch.Tensor] = None, rope_tokens: int = -1, across_heads: bool = False) -> torch.Tensor:
    """The differentiable, out-of-place norm + RoPE (routed.qk_norm_rope_autograd; the mutating vorta::qk_norm_rope has no
    gradient).  rope_tokens < 0: every token the tables cover.  Its autograd formula is vorta::qk_norm_rope_bwd."""
    from . import routed
    return routed._norm_rope_forward(x, weight, eps, cos, sin, None if rope_tokens < 0 else rope_tokens, across_heads)


@qk_norm_rope_grad.register_fake
def _(x, weight, eps, cos=None, sin=None, rope_tokens=-1, across_heads=False):
    return x.new_empty(x.shape)


@torch.library.custom_op("vorta::qk_norm_rope_bwd", mutates_args=(), device_types="cuda")
def qk_norm_rope_bwd(x: torch.Tensor, g: torch.Tensor, weight: Optional[torch.Tensor], eps: float,
                     cos: Optional[torch.Tensor] = None, sin: Optional[torch.Tensor] = None, rope_tokens: int = -1,
                     across_heads: bool = False, want_dweight: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dx, dweight) of vorta::qk_norm_rope_grad: vorta_qk_norm_rope_bwd.  dweight is float32 [D] / [H*D]; an empty tensor
    without a weight or with want_dweight=False (an operator returns tensors, not None)."""
    from . import routed
    dx, dw = routed._norm_rope_backward(x, g, weight, eps, cos, sin, None if rope_tokens < 0 else rope_tokens, across_heads,
                                        want_dweight and weight is not None)
    return dx, dw if dw is not None else x.new_empty((0,), dtype=torch.float32)


@qk_norm_rope_bwd.register_fake
def _(x, g, weight, eps, cos=None, sin=None, rope_tokens=-1, across_heads=False, want_dweight=True):
    n = weight.numel() if (want_dweight and weight is not None) else 0
    return torch.empty_like(x), x.new_empty((n,), dtype=torch.float32)


def _norm_rope_setup(ctx, inputs, output):
    x, weight, eps, cos, sin, rope_tokens, across_heads = inputs
    ctx.save_for_backward(x, weight, cos, sin)
    ctx.rest = (eps, rope_tokens, across_heads)


def _norm_rope_backward(ctx, g):
    x, weight, cos, sin = ctx.saved_tensors
    eps, rope_tokens, across_heads = ctx.rest
    want = weight is not None and ctx.needs_input_grad[1]
    dx, dw = torch.ops.vorta.qk_norm_rope_bwd(x, g, weight, eps, cos, sin, rope_tokens, across_heads, want)
    return dx, (dw.to(weight.dtype).view(weight.shape) if want else None), None, None, None, None, None


torch.library.register_autograd("vorta::qk_norm_rope_grad", _norm_rope_backward, setup_context=_norm_rope_setup)


@torch.library.custom_op("vorta::route_plan_", mutates_args=("scores", "expert", "lists", "counts"), device_types="cuda")
def route_plan_(temb: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, heads: int, tau: float, n_experts: int,
                scores: torch.Tensor, expert: torch.Tensor, lists: torch.Tensor, counts: torch.Tensor) -> None:
    """vorta_route_plan into caller-owned buffers at fixed addresses (patch/_engine.py RoutePlan; hipGraph replay)"""
    ops.route_plan(temb, weight, bias, heads, tau, n_experts, out=(scores, expert, lists, counts))


@route_plan_.register_fake
def _(temb, weight, bias, heads, tau, n_experts, scores, expert, lists, counts) -> None:
    return None


def geometry_args(lowres_group_info, window_size, tile_size, latent_shape) -> dict:
    """the geometry keywords of vorta::routed_attention / vorta::soft_mixture_attention from a processor's keywords"""
    return dict(latent=[int(x) for x in latent_shape], tile=[int(x) for x in tile_size], window=[int(x) for x in window_size],
                group=[int(x) for x in lowres_group_info.window_size], rate=float(lowres_group_info.reduction_rate))


def routing_args(head_routing) -> dict:
    """head_lists / head_counts / counts_host of a routed.HeadRouting"""
    return dict(head_lists=head_routing.lists, head_counts=head_routing.counts_dev,
                counts_host=None if head_routing.counts_host is None else [int(c) for c in head_routing.counts_host])
