"""The hard-routing (Eval) call body both models share: what `HunyuanVideoFlashAttnProcessorTripleEval.__call__` and
`WanAttnProcessorTripleEval.__call__` do between their projections and their output projections.

Where the routes come from (`resolve_routes`), first match: `route_rule` (the call's OWN measurement on batch item 0: tier routes
with the operands it prepared where the rule covers the precision, else a routing, its expert ids and the record; `route_sink`
receives one entry per call); a given `tier_routing` (a tier -> HeadRouting dictionary, or a routed.RepairableRoutes launched by
its views); `routing_score` / `tau_sparse` dispatched on the device (torch.ops.vorta.route_scores) when no `head_routing` is given;
the given `head_routing`.
How they are launched (`launch_routes`), one batch item per launch, first match: `repair_above` (item 0 is verified and repaired,
the tables in place; every other item launches the repaired tables without a verification of its own; `repair_sink` receives one
record per call and `fidelity` that record's rows as they were BEFORE the repair); tier routes (routed.routed_attention_tiers);
a `fidelity` / `expert_fidelity` sink (routed.routed_attention: a list is no operator argument); else the
torch.ops.vorta.routed_attention operator.  The operands a measurement prepared serve item 0 only: every other item converts its
own.  A model with text rows (Hunyuan, one item) passes `text_len` / `text_valid`; Wan passes neither.
"""
from typing import Any, NamedTuple, Optional

import torch

from .. import torch_ops as _torch_ops  # registers torch.ops.vorta.*
from .._partial import coreset_numbers, divides, partial_geometry
from ..routed import (HeadRouting, RepairableRoutes, TierRoutes, geometry_for, routed_attention_repaired,
                      routed_attention_tiers, tier_sink_entry)
from ..ulysses import SP_STATE


class EvalRoutes(NamedTuple):
    """what `resolve_routes` hands `launch_routes`"""
    head_routing: Optional[HeadRouting]   # the routing of the routed_attention rungs
    tier_routing: Optional[dict]          # tier -> HeadRouting: the call launches by precision tiers
    tier_operands: Optional[dict]         # tier -> AttnOperands a measurement prepared on item 0
    repairable: Any                       # the routes in the form routed.routed_attention_repaired verifies
    geom: Any = None                      # the RoutedGeometry, where a rule already looked it up


def check_eval_input(hidden_states, lowres_group_info, latent_shape, window_size, tile_size) -> None:
    """hunyuan.py:247-272 / wan.py:168-193 (same conditions, same messages).  With partial geometry switched on
    (set_partial_geometry) the two divisibility conditions fall away for a geometry that does not divide: one whole coreset window
    per dimension is needed, and a group info built for this latent shape.  A geometry that divides is checked as ever."""
    seq_length = hidden_states.shape[1] * SP_STATE.sp_size
    num_groups = lowres_group_info.center_indices.shape[0]
    group_size = lowres_group_info.center_indices.shape[1] + lowres_group_info.margin_indices.shape[1]
    if seq_length != latent_shape[0] * latent_shape[1] * latent_shape[2]:
        raise ValueError(f"Input sequence length {seq_length} does not match latent shape {latent_shape}.")
    if partial_geometry() and not divides(latent_shape, tile_size, lowres_group_info.window_size):
        # a partial geometry: the group info must still be the cropped windows of THIS latent shape
        want = coreset_numbers(latent_shape, lowres_group_info.window_size, lowres_group_info.reduction_rate)[0]
        if num_groups != want or tuple(lowres_group_info.latent_shape) != tuple(int(x) for x in latent_shape):
            raise ValueError(f"Low-res info {num_groups}x{group_size} was not built for latent shape {latent_shape} "
                             f"({want} whole windows).")
        return
    for t_size, l_size in zip(tile_size, latent_shape):
        if l_size % t_size != 0:
            raise ValueError(
                f"Tile size {tile_size} (dim={t_size}) does not divide latent shape {latent_shape} (dim={l_size}).")
    if seq_length != num_groups * group_size:
        raise ValueError(f"Input sequence length {seq_length} does not match low-res info {num_groups}x{group_size}.")


def refuse_under_sequence_parallel(expert_fidelity, route_rule, tier_routing, repair_above) -> None:
    """the keywords of an Eval call that do not run under sequence parallelism, refused by name"""
    if expert_fidelity is not None:
        raise NotImplementedError("sampled_expert_fidelity: the per-expert measurement on sampled rows does not run "
                                  "under sequence parallelism (its gather reads whole heads of one process)")
    if route_rule is not None:
        raise NotImplementedError("route_rule: routing by a measured error bound or FLOP budget does not run under "
                                  "sequence parallelism (its gather reads whole heads of one process)")
    if tier_routing is not None:
        raise NotImplementedError("tier_routing: launching by precision tiers does not run under sequence parallelism")
    if repair_above is not None:
        raise NotImplementedError("repair_above: verifying and repairing launched routes does not run under sequence "
                                  "parallelism (its dense repair launch reads whole heads of one process)")


def _item(b: int, *xs):
    """batch item `b` of (B,...) tensors as (1,...) views; of a batch of one the tensors themselves (no view is made)"""
    return xs if xs[0].shape[0] == 1 else tuple(x[b:b + 1] for x in xs)


def _text_kw(model: str, text_len: Optional[int], text_valid) -> dict:
    return dict(model=model) if text_len is None else dict(model=model, text_len=text_len, text_valid=text_valid)


def resolve_routes(q, k, v, geometry: dict, *, model: str, routing_score=None, tau_sparse=None,
                   head_routing: Optional[HeadRouting] = None, route_rule=None, route_sink: Optional[list] = None,
                   tier_routing=None, text_len: Optional[int] = None, text_valid=None) -> EvalRoutes:
    """The routes of one Eval call (the module docstring names the sources).  `geometry`: torch_ops.geometry_args of the call."""
    if route_rule is not None:
        geom = geometry_for(**geometry, device=q.device)
        # a batch is routed, every item, by ITEM 0's measurement (the reference's convention for scores: wan.py:388-416)
        routes = route_rule.route(*_item(0, q, k, v), geom, **_text_kw(model, text_len, text_valid))
        if isinstance(routes, TierRoutes):
            if route_sink is not None:
                route_sink.append(tier_sink_entry(routes))
            return EvalRoutes(None, routes.routings, routes.operands, routes, geom)
        head_routing, ids, fid = routes
        if route_sink is not None:
            route_sink.append((ids, head_routing.lists, head_routing.counts_dev, fid))
        # (a `tier_routing` given beside the rule: as it came)
        return EvalRoutes(head_routing, tier_routing, None, (head_routing, ids), geom)
    if tier_routing is not None:
        # (a RepairableRoutes holds the joint tables of the tiers: launched by their views)
        views = tier_routing.routings if isinstance(tier_routing, RepairableRoutes) else tier_routing
        return EvalRoutes(head_routing, views, None, tier_routing)
    if head_routing is None:  # top-1 / tau dispatch on the device: no torch.nonzero host sync (hunyuan.py:612-640)
        ids, lists, counts = torch.ops.vorta.route_scores(routing_score, float(tau_sparse))
        head_routing = HeadRouting.from_device(lists, counts, ids)
    return EvalRoutes(head_routing, None, None, head_routing)


def launch_routes(q, k, v, out, routes: EvalRoutes, geometry: dict, *, model: str, text_len: Optional[int] = None, text_valid=None,
                  fidelity: Optional[list] = None, fidelity_rows=None, fidelity_heads: str = "sparse",
                  expert_fidelity: Optional[list] = None, repair_above: Optional[float] = None,
                  repair_sink: Optional[list] = None) -> None:
    """Launch `resolve_routes`' routes on every batch item of (B,H,N,D) q, k, v into `out` (the module docstring names the
    rungs).  The geometry is looked up once, and only where a launcher takes the object: the operator takes `geometry` itself."""
    head_routing, tier_routing, geom = routes.head_routing, routes.tier_routing, routes.geom
    measured = fidelity is not None or expert_fidelity is not None
    if expert_fidelity is not None and repair_above is not None:
        raise ValueError("expert_fidelity: the per-expert sink does not go with repair_above")
    if expert_fidelity is not None and tier_routing is not None:
        raise ValueError("expert_fidelity: the per-expert sink does not go with a launch by precision tiers")
    if geom is None and (repair_above is not None or tier_routing is not None or measured):
        geom = geometry_for(**geometry, device=q.device)
    kw = _text_kw(model, text_len, text_valid)
    fkw = {} if fidelity is None else dict(fidelity=fidelity, fidelity_rows=fidelity_rows, fidelity_heads=fidelity_heads)
    for b in range(q.shape[0]):
        qb, kb, vb, ob = _item(b, q, k, v, out)
        operands = routes.tier_operands if b == 0 else None
        if repair_above is not None and b == 0:
            _, repaired = routed_attention_repaired(qb, kb, vb, routes.repairable, geom, repair_above=repair_above, rows=fidelity_rows,
                                                    operands=operands, out=ob, **kw)
            if repair_sink is not None:
                repair_sink.append(repaired)
            if fidelity is not None:  # (the rows as they were BEFORE the repair: the record the repair was decided by)
                fidelity.append(repaired.fidelity)
        elif repair_above is not None:
            # the tables are repaired in place, so every other item launches item 0's repaired heads dense
            routed_attention_repaired(qb, kb, vb, repaired.routes, geom, repair_above=None, out=ob, **kw, **fkw)
        elif tier_routing is not None:
            routed_attention_tiers(qb, kb, vb, tier_routing, geom, out=ob, operands=operands, **kw, **fkw)
        elif measured:
            # (a list is no operator argument: the launcher behind vorta::routed_attention, directly -- looked up per call)
            from ..routed import routed_attention
            routed_attention(qb, kb, vb, head_routing, geom, out=ob, fidelity=fidelity, fidelity_rows=fidelity_rows,
                             fidelity_heads=fidelity_heads, expert_fidelity=expert_fidelity, **kw)
        else:
            torch.ops.vorta.routed_attention(qb, kb, vb, ob, **_torch_ops.routing_args(head_routing), **geometry, **kw)
