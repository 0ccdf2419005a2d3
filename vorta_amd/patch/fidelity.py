"""Per-head expert fidelity of a patched transformer: is a router, or a `tau_sparse`, any good?

The routed method makes one claim per head: that head's sparse expert reproduces what full attention would have written.  The
training-time forward (the Train processors' soft mixture) holds the data that decides it -- all three expert outputs of every
head of the layer -- and `ops.expert_fidelity` (vorta_expert_fidelity: one deterministic pass, nothing materialised) reduces it
to per-head statistics.  The reference has no counterpart: its only signal is the end-to-end loss.

    with expert_fidelity(model):                      # every Train-processor call of a forward files its layer's statistics
        model(hidden_states, ..., self_attention_kwargs=kw)
    fid = fidelity_of(model)                          # ops.ExpertFidelity, stacked (L, H, ...); all ranks' heads under SP
    fid.rel_error()                                   # (L, H, 3): coreset, sliding tile, mixed output against full attention
    table = routes_from_fidelity(fid, 0.05)           # (L, H) experts: the cheapest within the bound -- no backward pass
    evaluate_routing(routing_scores_of(model), fid, geometry)   # what the router's own routes cost and lose

Expert ids are the processors': 0 full attention, 1 coreset, 2 sliding tile; columns 0 / 1 of the statistics are experts 1 / 2.

The above is the training-time forward, in 16 bits, at three times the routed step.  What an INFERENCE forward actually wrote --
hard top-1 routes with their `tau_sparse`, the 8-bit precisions, a partial geometry, a rank's heads -- is measured on a seeded
sample of video rows per head against dense attention in the input dtype (routed.routed_attention(fidelity=...),
vorta_sampled_fidelity), cheap enough to stay on during a generation:

    with routed_fidelity(model, n_rows=2048, seed=0, heads="sparse"):   # Eval processors: every routed call files its layer
        model(hidden_states, ..., self_attention_kwargs=kw)
    rf = routed_fidelity_of(model)                    # ops.SampledFidelity, stacked (L, H) + `expert` (L, H) as launched
    rf.rel_error()                                    # (L, H): NaN for heads that were not measured
    evaluate_routing(rf.expert, rf, geometry)         # a head's error is its measured one

What an inference forward COULD have written -- every expert of every head, on the same sample -- and a way to run by the answer:

    with sampled_expert_fidelity(model, n_rows=2048, seed=0):          # Eval processors: routed.sampled_expert_fidelity per layer
        model(hidden_states, ..., self_attention_kwargs=kw)
    fid = sampled_expert_fidelity_of(model)           # ops.ExpertFidelity (L, H, ...): coreset, sliding tile, the routed output
    table = routes_from_fidelity(fid, 0.05)           # the cheapest expert within the bound, per head
    with fixed_routes(model, table), routed_fidelity(model, heads="all"):
        model(hidden_states, ..., self_attention_kwargs=kw)            # launched by the table; routers and tau_sparse unread
    routed_fidelity_of(model).expert                  # == table

The same loop closed on the device -- every layer of every forward routed by its own measurement, by a stated rule:

    with measured_routes(model, max_rel_error=0.05, n_rows=512):       # or max_flops_share=0.4; no router, no tau_sparse, no host read
        model(hidden_states, ..., self_attention_kwargs=kw)            # routed.route_by_fidelity per layer (vorta_route_fidelity)
    experts, fid = measured_routes_of(model)          # (L, H) device table and the ExpertFidelity it came from

And with the bound over the 8-bit PRECISION of what is launched (process precision "i8pv", "fp8pv" or "auto8"):

    with measured_routes(model, max_rel_error=0.05, covers_precision=True):   # one measurement per precision tier, in its arithmetic
        model(hidden_states, ..., self_attention_kwargs=kw)            # routed.route_by_fidelity(tiers=...) (vorta_route_fidelity_tiers)
    tiers = measured_precisions_of(model)             # (L, H) global tier ids: 0 native, 1 fp8pv, 2 i8pv
    with fixed_routes(model, measured_routes_of(model)[0], precisions=tiers):   # the same launches, nothing measured
        model(hidden_states, ..., self_attention_kwargs=kw)

Or a BUDGET over the same pairs -- a time target: this share of the dense 16-bit layer's cost, any expert in any precision:

    with measured_routes(model, max_cost_share=0.4):                   # routes_within_cost_share is the rule (vorta_route_budget_tiers)
        model(hidden_states, ..., self_attention_kwargs=kw)
    measured_levels_of(model)                         # (L,) the error each layer's budget bought

And a bound on what every forward LAUNCHED -- stored routes between two measurements, a reused table, the 8-bit launches:

    with measured_routes(model, max_rel_error=0.05, refresh_every=4, repair_above=0.08):   # verify on the sampled rows, repair
        model(hidden_states, ..., self_attention_kwargs=kw)            # routed.routed_attention_repaired (vorta_route_repair)
    rel, state, experts, tiers = repaired_routes_of(model)             # (L, H): as checked | 0 / 1 kept / 2 repaired | after
    with fixed_routes(model, table, precisions=tiers, repair_above=0.08):   # `repair_routes` is the rule on the host
        model(hidden_states, ..., self_attention_kwargs=kw)
"""
from __future__ import annotations

import bisect
import contextlib
import math
from dataclasses import dataclass, field
from typing import Any, Dict, Mapping, NamedTuple, Optional, Tuple, Union

import torch
from torch import nn

from .. import _partial
from ..ops import ExpertFidelity, SampledFidelity
from ._engine import context_of

_COLUMN_OF_EXPERT = {1: 0, 2: 1}  # expert id -> column of sq_err / max_err / rel_error
_INF_PATTERN = 0x7F800000  # float32 +inf: non-negative float32 values order like their patterns below it


@contextlib.contextmanager
def expert_fidelity(model: nn.Module):
    """While active, every forward of `model` (patched with apply_vorta_transformer, Train processors) measures its layers:
    each soft-mixture call runs `ops.expert_fidelity` on its three expert outputs and its mixed output and files the result
    under its layer on that forward's `ForwardState` (a block recomputed under gradient checkpointing files the same bits
    again).  The flag is read once per forward, when it starts; teacher forwards (`original_attention`) measure nothing.
    Outside the context the forwards launch what they launch today."""
    ctx = context_of(model)
    if ctx.plan is None:
        raise ValueError("expert_fidelity: the model was not patched with apply_vorta_transformer")
    previous, ctx.measure_fidelity = ctx.measure_fidelity, True
    try:
        yield model
    finally:
        ctx.measure_fidelity = previous


def stack_fidelity(per_layer) -> ExpertFidelity:
    """a sequence of per-layer `ExpertFidelity` -> one with a leading layer axis"""
    per_layer = list(per_layer)
    first = per_layer[0]
    cat = lambda name: torch.stack([getattr(f, name) for f in per_layer])  # noqa: E731
    rng = None if any(f.range_ref is None for f in per_layer) else cat("range_ref")
    return ExpertFidelity(cat("sq_ref"), cat("max_ref"), cat("sq_err"), cat("max_err"), rng, first.n)


def fidelity_of(model: nn.Module) -> ExpertFidelity:
    """The statistics of the model's latest forward under `expert_fidelity(model)`, stacked over the layers in block order:
    sq_ref, max_ref (L, H); sq_err, max_err (L, H, 3).  Under sequence parallelism a rank measured its own heads over their
    whole sequences: they are all-gathered over the group here (a collective: every rank calls it) and range_ref is not
    carried.  Raises when no such forward is on record."""
    ctx = context_of(model)
    filed: Optional[Dict[int, ExpertFidelity]] = ctx.fidelity
    if not filed:
        raise RuntimeError("fidelity_of: no forward of this model has run under expert_fidelity(model) with soft-mixture "
                           "(Train) processors")
    fid = stack_fidelity(filed[layer] for layer in sorted(filed))
    from ..ulysses import SP_STATE
    if SP_STATE.enabled:
        from ..attention._sp import gather_fidelity
        fid = gather_fidelity(fid, ctx.plan.heads)
    return fid


@contextlib.contextmanager
def routed_fidelity(model: nn.Module, n_rows: int = 2048, seed: int = 0, heads: str = "sparse"):
    """While active, every forward of `model` (patched with apply_vorta_transformer, hard-routing Eval processors) measures
    the routed output it wrote: each routed self-attention call compares `n_rows` sampled video rows per head (the stratified
    table `routed.sample_rows(S, n_rows, seed)`; every row where the clip has fewer) with dense attention in the input dtype
    and files an `ops.SampledFidelity` under its layer.  heads: "sparse" = the heads routed to the coreset and sliding-tile
    experts, "all" = the full-attention heads as well (what an 8-bit precision costs them).  The flag is read once per
    forward, when it starts; teacher forwards (`original_attention`) measure nothing.  The forward stays free of host
    synchronisation and graph-capturable: the table is fixed, the gather, the launches and the compare run on the caller's
    stream.  Outside the context the forwards launch what they launch today.
    Together with `repair_above` (`measured_routes(..., repair_above=b)`, `fixed_routes(..., repair_above=b)`; the same
    (n_rows, seed): the two share one sample) the record reports the rows AS THEY WERE BEFORE THE REPAIR -- it is the record
    the repair was decided by, with `expert` the routes as launched -- and its heads are the verification's, whatever `heads`
    says: the sparse heads of the native tier, every head of an 8-bit tier."""
    from ..routed import FIDELITY_HEADS
    ctx = context_of(model)
    if ctx.plan is None:
        raise ValueError("routed_fidelity: the model was not patched with apply_vorta_transformer")
    if heads not in FIDELITY_HEADS or int(n_rows) < 0:
        raise ValueError(f"routed_fidelity: heads={heads!r} (one of {FIDELITY_HEADS}), n_rows={n_rows}")
    if ctx.measure_experts is not None and ctx.measure_experts != (int(n_rows), int(seed)):
        raise ValueError(f"routed_fidelity(n_rows={n_rows}, seed={seed}) inside sampled_expert_fidelity(n_rows="
                         f"{ctx.measure_experts[0]}, seed={ctx.measure_experts[1]}): the two share one sample")
    rule = None if ctx.measured_routes is None else ctx.measured_routes.rule
    if rule is not None and (rule.n_rows, rule.seed) != (int(n_rows), int(seed)):
        raise ValueError(f"routed_fidelity(n_rows={n_rows}, seed={seed}) inside measured_routes(n_rows={rule.n_rows}, "
                         f"seed={rule.seed}): the two share one sample")
    repair = ctx.route_repair
    if repair is not None and (repair.n_rows, repair.seed) != (int(n_rows), int(seed)):
        raise ValueError(f"routed_fidelity(n_rows={n_rows}, seed={seed}) inside a context with repair_above (n_rows="
                         f"{repair.n_rows}, seed={repair.seed}): the two share one sample")
    previous, ctx.measure_routed = ctx.measure_routed, (int(n_rows), int(seed), heads)
    try:
        yield model
    finally:
        ctx.measure_routed = previous


def stack_routed_fidelity(per_layer) -> SampledFidelity:
    """a sequence of per-layer `SampledFidelity` -> one with a leading layer axis (row_sq_err is not carried)"""
    per_layer = list(per_layer)
    first = per_layer[0]
    cat = lambda name: torch.stack([getattr(f, name) for f in per_layer])  # noqa: E731
    return SampledFidelity(cat("sq_ref"), cat("max_ref"), cat("sq_err"), cat("max_err"), cat("range_ref"), None, first.n,
                           first.rows, cat("expert"))


def routed_fidelity_of(model: nn.Module, item: int = 0) -> SampledFidelity:
    """The statistics of the model's latest forward under `routed_fidelity(model)`, stacked over the layers in block order:
    sq_ref, max_ref, sq_err, max_err, range_ref (L, H), `expert` (L, H) int32 = the head -> expert ids as launched, `rows` the
    sampled video tokens.  `item`: the batch item (Wan files one record per item).  Under sequence parallelism a rank measured
    its own heads: they are all-gathered over the group here (a collective: every rank calls it).  Raises when no such
    forward is on record."""
    ctx = context_of(model)
    filed = ctx.routed_fidelity
    if not filed:
        raise RuntimeError("routed_fidelity_of: no forward of this model has run under routed_fidelity(model) with "
                           "hard-routing (Eval) processors")
    fid = stack_routed_fidelity(filed[layer][item] for layer in sorted(filed))
    from ..ulysses import SP_STATE
    if SP_STATE.enabled:
        from ..attention._sp import gather_routed_fidelity
        fid = gather_routed_fidelity(fid)
    return fid


@contextlib.contextmanager
def sampled_expert_fidelity(model: nn.Module, n_rows: int = 2048, seed: int = 0):
    """While active, every forward of `model` (patched with apply_vorta_transformer, hard-routing Eval processors) measures
    what EACH expert would have written: after its routed launches, every routed self-attention call runs
    `routed.sampled_expert_fidelity` on `n_rows` sampled video rows per head (the table `routed.sample_rows(S, n_rows, seed)`,
    shared with `routed_fidelity(model)` when both are active -- they must then name the same sample) for every head, with
    `out=` the call's output, and files an `ops.ExpertFidelity` under its layer: column 0 coreset, column 1 sliding tile,
    column 2 the routed output as launched, all against dense attention in the input dtype.  The flag is read once per forward,
    when it starts; teacher forwards (`original_attention`) measure nothing.  No host read, graph-capturable; outside the
    context the forwards launch what they launch today.  Under sequence parallelism the measuring forward raises
    NotImplementedError by name (the gather reads whole heads of one process)."""
    ctx = context_of(model)
    if ctx.plan is None:
        raise ValueError("sampled_expert_fidelity: the model was not patched with apply_vorta_transformer")
    if int(n_rows) < 0:
        raise ValueError(f"sampled_expert_fidelity: n_rows={n_rows}")
    if ctx.measure_routed is not None and ctx.measure_routed[:2] != (int(n_rows), int(seed)):
        raise ValueError(f"sampled_expert_fidelity(n_rows={n_rows}, seed={seed}) inside routed_fidelity(n_rows="
                         f"{ctx.measure_routed[0]}, seed={ctx.measure_routed[1]}): the two share one sample")
    if ctx.measured_routes is not None:
        raise ValueError("sampled_expert_fidelity inside measured_routes: measured_routes runs that measurement itself "
                         "(measured_routes_of(model) returns its records)")
    previous, ctx.measure_experts = ctx.measure_experts, (int(n_rows), int(seed))
    try:
        yield model
    finally:
        ctx.measure_experts = previous


def sampled_expert_fidelity_of(model: nn.Module, item: int = 0) -> ExpertFidelity:
    """The records of the model's latest forward under `sampled_expert_fidelity(model)`, stacked over the layers in block
    order like `fidelity_of`'s: sq_ref, max_ref (L, H); sq_err, max_err (L, H, 3) -- `routes_from_fidelity` and
    `evaluate_routing` take it unchanged.  `item`: the batch item (Wan files one record per item)."""
    ctx = context_of(model)
    filed = ctx.sampled_experts
    if not filed:
        raise RuntimeError("sampled_expert_fidelity_of: no forward of this model has run under sampled_expert_fidelity(model) "
                           "with hard-routing (Eval) processors")
    return stack_fidelity(filed[layer][item] for layer in sorted(filed))


@contextlib.contextmanager
def fixed_routes(model: nn.Module, table, precisions=None, *, repair_above: Optional[float] = None, n_rows: int = 512,
                 seed: int = 0):
    """While active, the hard-routing (Eval) processors of `model` (patched with apply_vorta_transformer) launch the (L, H)
    expert `table` (0 full attention, 1 coreset, 2 sliding tile; e.g. `routes_from_fidelity`'s): every layer is routed by
    `HeadRouting.from_expert_ids(table[layer])`, with host counts, so an expert no head has launches nothing.  The routers'
    routes and `tau_sparse` are not consulted (a forward may leave `tau_sparse` out); `routed_fidelity_of(model).expert`
    reports the table.  The table is read once per forward, when it starts; teacher forwards stay dense.  Outside the context
    nothing changes.  ValueError for a table that is not (L, H) or holds another id.  Under sequence parallelism the context
    refuses by name (NotImplementedError): the head placement there follows `RoutePlan.experts_host`, which knows routers only.
    precisions: an (L, H) table of GLOBAL precision tier ids (0 native, 1 fp8pv, 2 i8pv; `measured_precisions_of(model)`'s):
    every head runs its expert in that tier (`routed.routed_attention_tiers`), whatever the process precision would have
    chosen for it.  ValueError for an id outside 0..2 and for a tier the process precision does not offer
    (`routed.TIERS_OF_PRECISION`, read when the context is entered).  None: every head in the process precision, as ever.
    repair_above: a bound >= 0 (None: nothing below applies, every forward launches what it launches today).  A reused table
    has no error bound of its own; with one, every forward VERIFIES what it launched on `n_rows` sampled video rows per head
    (`routed.sample_rows(S, n_rows, seed)`, the table shared with `routed_fidelity(model)`) and re-runs every head further than
    `repair_above` from dense attention, dense in the input dtype, in the same forward (`routed.routed_attention_repaired`;
    `repair_routes` is the rule).  The table is placed in DEVICE lists once per context entry and layer; a repaired head stays
    on full attention in the input dtype until the context exits (entering again starts from the table).
    `repaired_routes_of(model)` reads the latest forward's tables.  Refused by name: a negative or NaN bound; an 8-bit process
    precision without `precisions=` (the bound is on what is launched, so the routes must name the tier of every launch);
    sequence parallelism."""
    ctx = context_of(model)
    if ctx.plan is None:
        raise ValueError("fixed_routes: the model was not patched with apply_vorta_transformer")
    bound = _check_repair_above("fixed_routes", repair_above)
    if bound is not None:
        from ..routed import precision_of
        if int(n_rows) < 1:
            raise ValueError(f"fixed_routes: n_rows={n_rows} (at least 1: without a sampled row every error reads 0)")
        if precisions is None and precision_of(None) != "native":
            raise ValueError(f"fixed_routes: repair_above under the 8-bit process precision {precision_of(None)!r} needs tier "
                             "routes: give precisions= (measured_precisions_of(model)); a bound on what is launched has to route "
                             "over what is launched")
        if ctx.measure_routed is not None and ctx.measure_routed[:2] != (int(n_rows), int(seed)):
            raise ValueError(f"fixed_routes(repair_above=..., n_rows={n_rows}, seed={seed}) inside routed_fidelity(n_rows="
                             f"{ctx.measure_routed[0]}, seed={ctx.measure_routed[1]}): the two share one sample")
        if ctx.measure_experts is not None:
            raise ValueError("fixed_routes(repair_above=...) inside sampled_expert_fidelity: the per-expert sink does not go "
                             "with a repair")
    tier_table = None
    if precisions is not None:
        from ..routed import tiers_of
        from ..ops import TIER_NAMES
        p = torch.as_tensor(precisions).detach().cpu()
        if p.is_floating_point() or p.dtype == torch.bool or tuple(p.shape) != (len(ctx.plan), ctx.plan.heads):
            raise ValueError(f"fixed_routes: precisions: an integer tier table of shape ({len(ctx.plan)}, {ctx.plan.heads}) "
                             f"(layers, heads), got {tuple(p.shape)} {p.dtype}")
        if bool(((p < 0) | (p > 2)).any()):
            raise ValueError("fixed_routes: precision tier ids are 0 (native), 1 (fp8pv), 2 (i8pv)")
        offered = tiers_of(None)
        missing = sorted({TIER_NAMES[int(x)] for x in p.flatten().tolist()} - set(offered))
        if missing:
            raise ValueError(f"fixed_routes: precisions name {missing}, which the process precision does not offer (its tiers: "
                             f"{offered}; set_attention_precision)")
        tier_table = [[int(x) for x in row] for row in p.tolist()]
    t = torch.as_tensor(table).detach().cpu()
    L, H = len(ctx.plan), ctx.plan.heads
    if t.is_floating_point() or t.dtype == torch.bool or tuple(t.shape) != (L, H):
        raise ValueError(f"fixed_routes: an integer expert table of shape ({L}, {H}) (layers, heads), got "
                         f"{tuple(t.shape)} {t.dtype}")
    if bool(((t < 0) | (t > 2)).any()):
        raise ValueError("fixed_routes: expert ids are 0 (full), 1 (coreset), 2 (sliding tile)")
    if ctx.measured_routes is not None:
        raise ValueError("fixed_routes inside measured_routes: a forward is routed by the table or by the measurement, not both")
    from ..ulysses import SP_STATE
    if SP_STATE.enabled:
        raise NotImplementedError("fixed_routes: routing by a table does not run under sequence parallelism")
    previous, ctx.fixed_routes = ctx.fixed_routes, [[int(x) for x in row] for row in t.tolist()]
    previous_tiers, ctx.fixed_precisions = ctx.fixed_precisions, tier_table
    previous_repair = ctx.route_repair
    if bound is not None:
        ctx.route_repair = RouteRepair(bound, int(n_rows), int(seed))
    try:
        yield model
    finally:
        ctx.fixed_routes, ctx.fixed_precisions = previous, previous_tiers
        if bound is not None:
            ctx.route_repair, ctx.latest_route_repair = previous_repair, ctx.route_repair


@dataclass(eq=False)
class RouteRepair:
    """The state of one context with `repair_above`: the bound, the sample, per layer the device tables a `fixed_routes`
    table was placed in (they hold the repairs until the context exits) and the record of the latest forward's call"""
    bound: float
    n_rows: int = 512
    seed: int = 0
    tables: Dict[int, Any] = field(default_factory=dict)    # layer -> routed.RepairableRoutes (fixed_routes)
    latest: Dict[int, Any] = field(default_factory=dict)    # layer -> routed.RepairRecord of the latest forward

    def rows(self, latent_shape, device) -> torch.Tensor:
        from ..routed import sample_rows
        S = 1
        for x in latent_shape:
            S *= int(x)
        return sample_rows(S, min(self.n_rows, S), self.seed, device)

    def fixed_tables(self, layer: int, experts, tiers, device):
        """the layer's rows of a `fixed_routes` table as device tables, built once per context entry: under one `native`
        tier without `tiers` (the global tier ids of `precisions=`), else over the tiers the row names and `native`, the
        cheapest first as `fixed_routes` launches them"""
        if layer not in self.tables:
            from ..ops import TIER_NAMES
            from ..routed import HeadRouting, RepairableRoutes
            i32 = lambda x: torch.tensor(x, dtype=torch.int32).to(device)  # noqa: E731
            if tiers is None:
                routing = HeadRouting.from_expert_ids(experts, device)
                made = RepairableRoutes(("native",), i32(list(experts)), None, routing.lists.view(1, 3, len(experts)),
                                        i32([routing.counts_host]))
            else:
                order = sorted(set(tiers) | {0}, reverse=True)
                per = [HeadRouting.from_expert_ids([e if p == t else -1 for e, p in zip(experts, tiers)], device) for t in order]
                made = RepairableRoutes(tuple(TIER_NAMES[t] for t in order), i32(list(experts)),
                                        i32([order.index(t) for t in tiers]), torch.stack([r.lists for r in per]),
                                        i32([r.counts_host for r in per]))
            self.tables[layer] = made
        return self.tables[layer]

    def file(self, layer: int, record) -> None:
        self.latest[layer] = record


def _check_repair_above(who: str, repair_above) -> Optional[float]:
    if repair_above is None:
        return None
    if isinstance(repair_above, (bool, str)) or not float(repair_above) >= 0:
        raise ValueError(f"{who}: repair_above={repair_above!r} (a bound >= 0, or None: a negative or NaN bound keeps no head)")
    return float(repair_above)


@dataclass(eq=False)
class MeasuredRoutes:
    """The state of one `measured_routes(model, ...)` context: its rule, its count of the model's non-teacher forwards, and
    per layer what the latest measuring forward filed -- the processors' sink entries (expert_ids, lists, counts, fid)"""
    rule: Any                       # routed.RouteRule
    refresh_every: int = 1
    forwards: int = 0
    filed: Dict[int, list] = field(default_factory=dict)
    repairable: Dict[int, Any] = field(default_factory=dict)   # layer -> routed.RepairableRoutes of `filed` (stored_repairable)

    def begin_forward(self) -> bool:
        """counts a forward; True where it measures: forwards 0, k, 2k, ... of the context"""
        measures = self.forwards % self.refresh_every == 0
        self.forwards += 1
        return measures

    def file(self, layer: int, entries: list) -> None:
        self.filed[layer] = entries
        self.repairable.pop(layer, None)

    def stored_routing(self, layer: int):
        """the device lists and counts the latest measuring forward stored for `layer`, as a HeadRouting: nothing is launched"""
        from ..routed import HeadRouting
        entries = self.filed.get(layer)
        if not entries:  # (never with the patch's own forwards: every routed layer of a measuring forward files its lists)
            raise RuntimeError(f"measured_routes: layer {layer} has no measured routes on record for a forward between two "
                               "measurements (the latest measuring forward did not run this layer's self-attention)")
        if len(entries[0]) > 4:
            raise RuntimeError(f"measured_routes: layer {layer} stored routes over precision tiers (stored_tier_routing)")
        return HeadRouting.from_device(entries[0][1], entries[0][2], entries[0][0])

    def stored_repairable(self, layer: int):
        """the joint device tables the latest measuring forward stored for `layer`, routed over precision tiers, as ONE
        routed.RepairableRoutes -- made once per measurement, so that what a forward repairs in place (the caller's tier index
        included) is what the next one launches"""
        from ..routed import RepairableRoutes
        if layer not in self.repairable:
            ids, lists, counts, _, data = self.filed[layer][0]
            from ..ops import TIER_NAMES
            index = torch.zeros_like(data["tier_ids"])
            for i, name in enumerate(data["tiers"]):
                index = torch.where(data["tier_ids"] == TIER_NAMES.index(name), i, index)
            self.repairable[layer] = RepairableRoutes(tuple(data["tiers"]), ids, index.to(torch.int32), lists, counts,
                                                      data["tier_ids"])
        return self.repairable[layer]

    def stores_tiers(self, layer: int) -> bool:
        """whether the latest measuring forward routed `layer` over precision tiers (a 5-tuple in the sink)"""
        entries = self.filed.get(layer)
        return bool(entries) and len(entries[0]) > 4

    def stored_tier_routing(self, layer: int):
        """tier -> HeadRouting of the device lists and counts the latest measuring forward stored for `layer`, in its launch
        order: nothing is launched"""
        from ..routed import HeadRouting
        _, lists, counts, _, data = self.filed[layer][0]
        return {name: HeadRouting.from_device(lists[i], counts[i]) for i, name in enumerate(data["tiers"])}


@contextlib.contextmanager
def measured_routes(model: nn.Module, *, max_rel_error: Optional[float] = None, max_flops_share: Optional[float] = None,
                    n_rows: int = 512, seed: int = 0, refresh_every: int = 1, covers_precision: bool = False,
                    tier_cost: Optional[Mapping] = None, repair_above: Optional[float] = None,
                    max_cost_share: Optional[float] = None):
    """While active, every non-teacher forward of `model` (patched with apply_vorta_transformer, hard-routing Eval processors)
    routes each layer by a MEASUREMENT of that layer on its own q, k, v, held per prompt, per layer and per step, without a
    router checkpoint and without a host read (`routed.route_by_fidelity`: `n_rows` sampled video rows per head,
    `routed.sample_rows(S, n_rows, seed)`; then vorta_route_fidelity).  Exactly one rule:
    `max_rel_error=b`: no sparse head is further than b from dense attention on the sampled rows -- per head the cheapest
    expert within the bound, full attention where none is; `max_flops_share=s`: per layer at most the share s of the all-dense
    FLOPs, spent where it hurts least (`routes_from_fidelity` defines both).  The bound covers the sampled rows and the METHOD:
    the measurement runs in the dtype of q, k, v, whatever 8-bit precision the routed launches use -- unless
    `covers_precision=True` (with `max_rel_error`; with `max_flops_share` a ValueError by name): every layer is then measured
    once per precision tier of the process precision (`routed.TIERS_OF_PRECISION`: "i8pv" -> i8pv, native; "fp8pv" -> fp8pv,
    native; "auto8" -> i8pv, fp8pv, native) IN that tier's precision, routed over (tier, expert) pairs -- per head the
    cheapest within the bound, cost = work[expert] * tier_cost[tier] (`routes_from_fidelity_tiers` is the rule; `tier_cost`
    None: `ops.DEFAULT_TIER_COST`), full attention in the input dtype where none is -- and launched tier by tier
    (`routed.routed_attention_tiers`).  The bound then holds for the candidate launches on the sampled rows, precision
    included; a full-size launch is the same arithmetic with another key cut and, under "i8pv", another grouping of rows into
    waves.  Under "native" the flag changes nothing.  `measured_precisions_of(model)` reads the tiers back.
    `refresh_every=k`: the context counts the model's non-teacher forwards on the host and measures on forwards 0, k, 2k, ...
    of the context; between them every layer launches the device lists and counts it stored (`HeadRouting.from_device`),
    with nothing measured or launched beyond the routed call.  A pipeline that runs two forwards per step (Wan's
    classifier-free guidance) counts two: with k = 2 the conditional forward measures and the unconditional one launches its
    routes.  The routers' routes, `tau_sparse` (a forward may leave it out) and `head_routing` are not consulted; teacher
    forwards stay dense.  Inside `routed_fidelity(model)` with the same (n_rows, seed) -- the two share one sample -- that
    record's `expert` reports the measured routes.  Outside the context nothing changes.
    `repair_above=b` (None: nothing of this applies): every non-teacher forward in the context -- the measuring ones and
    the ones that launch stored routes -- VERIFIES every routed self-attention call on the context's sample (`n_rows`, `seed`)
    and re-runs every head whose launched output is further than b from dense attention, dense in the input dtype, in the
    same forward (`routed.routed_attention_repaired`; `repair_routes` is the rule).  The repair is written into the stored
    device tables: the forwards up to the next measurement launch a repaired head dense, and a measuring forward writes fresh
    tables.  The bound then covers what was LAUNCHED on the sampled rows -- stale routes between two measurements and the
    8-bit precision of the launches included -- where `max_rel_error` covers the candidates of a measuring forward; under
    `max_flops_share` it is the only error bound there is.  `repaired_routes_of(model)` reads the latest forward's tables;
    `measured_routes_of(model)` then reports the experts after the repairs.
    `max_cost_share=s`, the third rule: a budget that covers the precision -- per layer at most the share s of what the layer
    costs with every head on full attention in the input dtype, spent on ANY expert in ANY tier of the process precision so
    that the largest per-head error is as small as that buys (`routes_within_cost_share` is the rule; vorta_route_budget_tiers
    applies it).  `covers_precision` is implied -- one measurement per tier, launched tier by tier, as above -- and
    `tier_cost`, `refresh_every` and `repair_above` work as for the bound over tiers; under "native" the one tier is routed.
    `measured_levels_of(model)` reads the error each layer's budget bought.  A time target, not an error target: where
    `max_flops_share` cannot spend on the 8-bit kernels, this rule can.
    Refused by name: a model that was not patched; more than one rule or none; nesting with `fixed_routes`, `sampled_expert_fidelity`
    or another `measured_routes`, either way round; sequence parallelism (NotImplementedError, as `fixed_routes`); a negative or
    NaN `repair_above`; `repair_above` under an 8-bit process precision without `covers_precision=True` (the bound is on what
    is launched, so the routes must name the tier of every launch)."""
    from ..routed import ROUTE_RULE_MODES, RouteRule
    ctx = context_of(model)
    if ctx.plan is None:
        raise ValueError("measured_routes: the model was not patched with apply_vorta_transformer")
    if covers_precision and max_flops_share is not None:
        raise ValueError("measured_routes: covers_precision with max_flops_share: a FLOP budget has no form over precision "
                         "tiers; give max_rel_error")
    covers_precision = bool(covers_precision) or max_cost_share is not None  # (the cost budget implies it)
    if tier_cost is not None and not covers_precision:
        raise ValueError("measured_routes: tier_cost goes with covers_precision=True")
    if sum(x is not None for x in (max_rel_error, max_flops_share, max_cost_share)) != 1:
        raise ValueError("measured_routes: exactly one of max_rel_error and max_flops_share and max_cost_share")
    if covers_precision:
        from ..ops import tier_plan
        tier_plan({"native": None}, tier_cost)  # (ValueError for a tier that is none of the three, a cost not positive and finite)
        tier_cost = None if tier_cost is None else dict(tier_cost)
    mode, given = next((m, x) for m, x in zip(ROUTE_RULE_MODES, (max_rel_error, max_flops_share, max_cost_share)) if x is not None)
    value = float(given)
    if not (value >= 0 if mode == ROUTE_RULE_MODES[0] else value > 0):
        raise ValueError(f"measured_routes: {mode}={value} (a bound >= 0; a share > 0)")
    if not ctx.needs_tau:
        raise ValueError("measured_routes: the model was patched with soft-mixture (Train) processors, which run every "
                         "expert of every head: only the hard-routing (Eval) processors are routed")
    if int(n_rows) < 1 or int(refresh_every) < 1:
        raise ValueError(f"measured_routes: n_rows={n_rows}, refresh_every={refresh_every} (both at least 1: without a "
                         "sampled row every error reads 0 and every head would meet any bound)")
    if ctx.fixed_routes is not None:
        raise ValueError("measured_routes inside fixed_routes: a forward is routed by the table or by the measurement, not both")
    if ctx.measure_experts is not None:
        raise ValueError("measured_routes inside sampled_expert_fidelity: measured_routes runs that measurement itself "
                         "(measured_routes_of(model) returns its records)")
    if ctx.measured_routes is not None:
        raise ValueError("measured_routes inside measured_routes: one rule routes a forward")
    if ctx.measure_routed is not None and ctx.measure_routed[:2] != (int(n_rows), int(seed)):
        raise ValueError(f"measured_routes(n_rows={n_rows}, seed={seed}) inside routed_fidelity(n_rows="
                         f"{ctx.measure_routed[0]}, seed={ctx.measure_routed[1]}): the two share one sample")
    from ..ulysses import SP_STATE
    if SP_STATE.enabled:
        raise NotImplementedError("measured_routes: routing by a measurement does not run under sequence parallelism")
    bound = _check_repair_above("measured_routes", repair_above)
    if bound is not None:
        from ..routed import precision_of
        if not covers_precision and precision_of(None) != "native":
            raise ValueError(f"measured_routes: repair_above under the 8-bit process precision {precision_of(None)!r} needs tier "
                             "routes: give covers_precision=True; a bound on what is launched has to route over what is launched")
    ctx.measured_routes = MeasuredRoutes(RouteRule(mode, value, int(n_rows), int(seed), bool(covers_precision), tier_cost, bound),
                                         int(refresh_every))
    previous_repair = ctx.route_repair
    if bound is not None:
        ctx.route_repair = RouteRepair(bound, int(n_rows), int(seed))
    try:
        yield model
    finally:
        ctx.measured_routes, ctx.latest_measured_routes = None, ctx.measured_routes
        if bound is not None:
            ctx.route_repair, ctx.latest_route_repair = previous_repair, ctx.route_repair


def measured_routes_of(model: nn.Module, item: int = 0) -> Tuple[torch.Tensor, ExpertFidelity]:
    """(experts, fid) of the model's latest MEASURING forward under `measured_routes(model, ...)`, stacked over the layers in
    block order: `experts` the (L, H) int32 head -> expert table on the device (read only when asked: `fixed_routes(model,
    experts)` reads it), `fid` the `ops.ExpertFidelity` (L, H, ...) the routes came from (column 2 NaN) -- `evaluate_routing`
    and `routes_from_fidelity` take it unchanged.  `item`: the batch item that was measured; a call measures item 0 alone
    (Wan routes a batch by it), so 0."""
    ctx = context_of(model)
    measured = ctx.measured_routes if ctx.measured_routes is not None else ctx.latest_measured_routes
    if measured is None or not measured.filed:
        raise RuntimeError("measured_routes_of: no forward of this model has measured under measured_routes(model, ...) with "
                           "hard-routing (Eval) processors")
    entries = [measured.filed[layer][item] for layer in sorted(measured.filed)]
    return torch.stack([e[0] for e in entries]), stack_fidelity(e[3] for e in entries)


def repaired_routes_of(model: nn.Module) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(rel, state, experts, tiers) of the model's latest forward inside a context with `repair_above`
    (`measured_routes(..., repair_above=b)`, `fixed_routes(..., repair_above=b)`), each (L, H) on the device, layers in block
    order: `rel` float32, the error of every head AS CHECKED (as launched, before the repair; NaN for a head that was not
    checked); `state` int32, 0 not checked (its launch is full attention in the input dtype), 1 kept, 2 repaired by that
    forward; `experts` int32, the head -> expert table AFTER the repair, and `tiers` int32, the GLOBAL precision tier ids
    (0 native, 1 fp8pv, 2 i8pv) after it.  The two tables are the live ones: read them before the next forward runs."""
    from ..ops import TIER_NAMES
    ctx = context_of(model)
    repair = ctx.route_repair if ctx.route_repair is not None else ctx.latest_route_repair
    if repair is None or not repair.latest:
        raise RuntimeError("repaired_routes_of: no forward of this model has run inside measured_routes(model, ..., "
                           "repair_above=...) or fixed_routes(model, ..., repair_above=...) with hard-routing (Eval) processors")
    records = [repair.latest[layer] for layer in sorted(repair.latest)]
    tiers = []
    for r in records:
        routes = r.routes
        if routes.tier_index is None:
            tiers.append(torch.zeros_like(routes.expert_ids))
        else:
            ids = torch.tensor([TIER_NAMES.index(name) for name in routes.tiers], dtype=torch.int32).to(routes.expert_ids.device)
            tiers.append(ids[routes.tier_index.long()])
    return (torch.stack([r.rel for r in records]), torch.stack([r.state_of_head for r in records]),
            torch.stack([r.routes.expert_ids for r in records]), torch.stack(tiers))


def measured_precisions_of(model: nn.Module, item: int = 0) -> torch.Tensor:
    """The (L, H) int32 table of GLOBAL precision tier ids (0 native, 1 fp8pv, 2 i8pv) of the model's latest MEASURING forward
    under `measured_routes(model, ..., covers_precision=True)`, on the device, layers in block order: the tier every head was
    launched in, beside `measured_routes_of(model)[0]`, its expert -- `fixed_routes(model, experts, precisions=...)` replays
    the pair.  A layer that was routed over experts alone (without the flag, or under the "native" process precision) reads 0
    throughout: every head in the process precision."""
    ctx = context_of(model)
    measured = ctx.measured_routes if ctx.measured_routes is not None else ctx.latest_measured_routes
    if measured is None or not measured.filed:
        raise RuntimeError("measured_precisions_of: no forward of this model has measured under measured_routes(model, ...) "
                           "with hard-routing (Eval) processors")
    entries = [measured.filed[layer][item] for layer in sorted(measured.filed)]
    return torch.stack([e[4]["tier_ids"] if len(e) > 4 else torch.zeros_like(e[0]) for e in entries])


def measured_levels_of(model: nn.Module, item: int = 0) -> torch.Tensor:
    """The (L,) float32 levels of the model's latest MEASURING forward under `measured_routes(model, max_cost_share=...)`, on
    the device, layers in block order: per layer the error its budget bought (`routes_within_cost_share`'s `level`) -- every
    head that had a qualifying candidate is within it on the sampled rows.  RuntimeError where the latest measuring forward
    was routed by another rule: a bound states its own error, and a FLOP budget buys none that is on record."""
    ctx = context_of(model)
    measured = ctx.measured_routes if ctx.measured_routes is not None else ctx.latest_measured_routes
    if measured is None or not measured.filed:
        raise RuntimeError("measured_levels_of: no forward of this model has measured under measured_routes(model, ...) "
                           "with hard-routing (Eval) processors")
    entries = [measured.filed[layer][item] for layer in sorted(measured.filed)]
    if any(len(e) <= 4 or e[4].get("level") is None for e in entries):
        raise RuntimeError("measured_levels_of: the latest measuring forward was not routed by max_cost_share")
    return torch.cat([e[4]["level"].reshape(1) for e in entries])


Geometry = Union[Mapping[str, Any], Any]


def _geometry_numbers(geometry: Geometry) -> Tuple[int, int, int, float]:
    """(S, S_low, tokens per full tile, keys a sliding-tile query sees among the video tokens) of a `routed.RoutedGeometry` or of
    a mapping with latent / tile / window / group / rate (or the self_attention_kwargs spelling: latent_shape, tile_size,
    window_size, lowres_group_info)"""
    if isinstance(geometry, Mapping):
        g = dict(geometry)
        latent = g.get("latent", g.get("latent_shape"))
        tile = g.get("tile", g.get("tile_size"))
        window = g.get("window", g.get("window_size"))
        info = g.get("lowres_group_info")
        group = g.get("group", None if info is None else info.window_size)
        rate = g.get("rate", None if info is None else info.reduction_rate)
        partial = _partial.partial_geometry()  # a mapping follows the process-wide switch, as the geometry it names would
    else:
        partial = getattr(geometry, "is_partial", False)
        latent, tile, window, group, rate = geometry.latent, geometry.tile, geometry.window, geometry.group, geometry.rate
    if any(x is None for x in (latent, tile, window, group, rate)):
        raise ValueError("geometry needs latent, tile, window, group and rate")
    S = int(latent[0]) * int(latent[1]) * int(latent[2])
    tok = int(tile[0]) * int(tile[1]) * int(tile[2])
    if partial and not _partial.divides(latent, tile, group):
        # a partial geometry (with the switch off the figures stay what they were): S_low counts the remainder tokens, and the sliding keys differ per query tile --
        # their mean over the video queries, so that S * keys is the true number of (query, key) pairs
        return S, _partial.coreset_numbers(latent, group, rate)[3], tok, _partial.sliding_video_pairs(latent, tile, window) / S
    gsz = int(group[0]) * int(group[1]) * int(group[2])
    s_low = (S // gsz) * int(gsz * (1 - float(rate)))
    n_kv = 1
    for l, t, w in zip(latent, tile, window):
        n_kv *= min(int(l) // int(t), int(w))
    return S, s_low, tok, n_kv * tok


def expert_work(geometry: Geometry, text_valid: int = 0, head_dim: int = 128) -> Tuple[float, float, float]:
    """FLOPs of one head under expert 0 / 1 / 2 by the work formulas of BASELINE.md section 2:
    F_full = 4 (S + T_eff)^2 D, F_low = 4 (S_low + T_eff)^2 D, F_sl = 4 D [S (n_kv tok + T_eff) + T_eff (S + T_eff)].
    A mapping with `work` names the three figures itself (measured costs, say): they are returned as they are."""
    if isinstance(geometry, Mapping) and geometry.get("work") is not None:
        work = tuple(float(x) for x in geometry["work"])
        if len(work) != 3 or not all(x > 0 and math.isfinite(x) for x in work):
            raise ValueError("geometry['work']: three positive finite figures (expert 0 / 1 / 2)")
        return work
    S, s_low, _, keys = _geometry_numbers(geometry)
    te, D = int(text_valid), int(head_dim)
    return (4.0 * (S + te) ** 2 * D, 4.0 * (s_low + te) ** 2 * D, 4.0 * D * (S * (keys + te) + te * (S + te)))


def _routes_within_budget(rel: torch.Tensor, work: Tuple[float, float, float], max_flops_share: float) -> torch.Tensor:
    """`routes_from_fidelity(max_flops_share=...)` on a CPU float32 rel (..., H, 3): plain Python per layer, in doubles"""
    w0, w1, w2 = (float(x) for x in work)
    H = rel.shape[-2]
    flat = rel.reshape(-1, H, rel.shape[-1])
    table = torch.zeros(flat.shape[:2], dtype=torch.int64)
    budget = float(max_flops_share) * (H * w0)
    for layer, rows in enumerate(flat.tolist()):
        ranking = []  # (rel of the candidate, head, candidate)
        for h, row in enumerate(rows):
            # (rel, work, -expert): the smaller rel, then the smaller work, then expert 2
            cands = [(row[_COLUMN_OF_EXPERT[e]], work[e], -e) for e in (1, 2)
                     if work[e] < w0 and math.isfinite(row[_COLUMN_OF_EXPERT[e]])]
            if cands:
                r, _, neg_e = min(cands)
                ranking.append((r, h, -neg_e))
        ranking.sort(key=lambda x: x[:2])
        n = [H, 0, 0]
        for _, h, e in ranking:
            # from the integer counts, left to right: the order of the moves cannot change the bits
            if not (n[0] * w0 + n[1] * w1 + n[2] * w2 > budget):
                break
            n[0] -= 1
            n[e] += 1
            table[layer, h] = e
    return table.reshape(rel.shape[:-1])


def routes_from_fidelity(fid: ExpertFidelity, max_rel_error: Optional[float] = None, geometry: Optional[Geometry] = None,
                         text_valid: int = 0, *, max_flops_share: Optional[float] = None) -> torch.Tensor:
    """(..., H) int64 expert table (on the CPU) by ONE of two rules (both or neither: ValueError).
    `max_rel_error`: per head the CHEAPEST expert whose `rel_error` is within `max_rel_error`
    (<=), full attention (0) where no sparse expert meets it.  Cost order: sliding tile, coreset, full -- the order the work
    formulas of BASELINE.md give at every published geometry; with `geometry` the order is computed from them (`expert_work`).
    A tie takes the cheaper expert.  A NaN error meets no bound.  No backward pass, no router: a table to compare a router's
    routes against, or to route by.
    `max_flops_share` (needs `geometry`): spend at most that share of the all-dense layer's FLOPs where it hurts least, per
    layer.  A head's candidate is the sparse expert with the smaller rel.  Only experts with work[e] < work[0] and a finite rel
    count.  On equal rel, take the smaller work, then expert 2.  A head with no such expert has no candidate.  Heads are
    ranked by (rel of candidate, head id) ascending.  Start with every head on expert 0.  Walk the ranking.  While
    cost > max_flops_share * (heads * work[0]), move the next head to its candidate.  cost = n0*work[0] + n1*work[1] +
    n2*work[2], evaluated in double from the integer counts, left to right.  Stop when the cost is within the budget or the
    candidates run out; max_flops_share >= 1 moves nothing.
    This function is the definition of both rules: `ops.route_fidelity` (vorta_route_fidelity) applies them on the device."""
    if (max_rel_error is None) == (max_flops_share is None):
        raise ValueError("routes_from_fidelity: exactly one of max_rel_error and max_flops_share")
    rel = fid.rel_error().detach().cpu()
    if max_flops_share is not None:
        if geometry is None:
            raise ValueError("routes_from_fidelity: max_flops_share needs `geometry` (the work of the experts: expert_work)")
        share = float(max_flops_share)
        if not share > 0:
            raise ValueError(f"routes_from_fidelity: max_flops_share={max_flops_share} (a positive share)")
        return _routes_within_budget(rel.float(), expert_work(geometry, text_valid), share)
    order = (2, 1)  # sparse experts, cheapest first
    if geometry is not None:
        work = expert_work(geometry, text_valid)
        order = tuple(sorted((1, 2), key=lambda e: (work[e], -e)))
    table = torch.zeros(rel.shape[:-1], dtype=torch.int64)
    for e in reversed(order):  # the cheapest is written last: it wins a tie
        table = torch.where(rel[..., _COLUMN_OF_EXPERT[e]] <= float(max_rel_error), torch.full_like(table, e), table)
    return table


def routes_from_fidelity_tiers(fids, max_rel_error: Optional[float] = None, geometry: Optional[Geometry] = None,
                               text_valid: int = 0, *, tier_cost: Optional[Mapping] = None,
                               max_flops_share: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(experts, tiers), two (..., H) int64 tables (on the CPU): per head the expert AND the precision tier to launch it in,
    from one record per tier.  `fids`: a mapping tier -> ExpertFidelity in the caller's order, cheapest first; a tier is
    named `native` / `fp8pv` / `i8pv` or by its global id 0 / 1 / 2 (`ops.TIER_NAMES`), and `tiers` holds the global ids.  Tier
    t's record holds what the coreset (column 0), the sliding tile (column 1) and FULL ATTENTION (column 2) write in that
    tier's precision against dense attention in the input dtype (`routed.sampled_expert_fidelity(precision=...)`); sq_ref is
    the first record's.  `native`'s full attention is that reference: its column 2 is not read and counts as 0.
    The rule.  A candidate is a pair (tier index t, expert e) with rel = `rel_error` of its column, in float32, and
    cost = work[e] * tier_cost[tier], one product in double; work = `expert_work(geometry, text_valid)`, (3, 2, 1) without a
    geometry; `tier_cost` a mapping tier -> cost (None: `ops.DEFAULT_TIER_COST`).  Per head take the cheapest candidate with
    rel <= max_rel_error (compared in float32; NaN meets no bound); on equal cost the lower tier index, then the larger
    expert id; where no candidate qualifies, full attention in the LAST tier.
    ValueError for `max_flops_share` (by name: a FLOP budget has no tier form), for a tier that is none of the three or named
    twice, and for a `tier_cost` that is not positive and finite for a tier in use.
    This function is the definition: `ops.route_fidelity_tiers` (vorta_route_fidelity_tiers) applies it on the device."""
    from ..ops import DEFAULT_ROUTE_WORK, tier_plan
    if max_flops_share is not None:
        raise ValueError("routes_from_fidelity_tiers: max_flops_share has no form over precision tiers (a FLOP budget routes "
                         "experts alone: routes_from_fidelity); give max_rel_error")
    if max_rel_error is None or not float(max_rel_error) >= 0:
        raise ValueError(f"routes_from_fidelity_tiers: max_rel_error={max_rel_error} (a bound >= 0)")
    ids, costs, exact = tier_plan(fids, tier_cost)
    work = DEFAULT_ROUTE_WORK if geometry is None else expert_work(geometry, text_valid)
    bound = float(torch.tensor(float(max_rel_error), dtype=torch.float32))  # the comparison is float32's
    records = list(fids.values())
    sq_ref = records[0].sq_ref.detach().cpu().float()
    rels = []  # per tier (N, H, 3) float32 as Python doubles
    for f in records:
        sq_err = f.sq_err.detach().cpu().float()
        rel = ExpertFidelity(sq_ref, sq_ref, sq_err, sq_err).rel_error()
        rels.append(rel.reshape(-1, rel.shape[-2], 3).tolist())
    shape = tuple(records[0].sq_err.shape[:-1])
    N, H, T = len(rels[0]), shape[-1], len(ids)
    experts = torch.zeros((N, H), dtype=torch.int64)
    tiers = torch.zeros((N, H), dtype=torch.int64)
    for layer in range(N):
        for h, (t, e) in enumerate(_pairs_within_bound([rels[t][layer] for t in range(T)], bound, work, costs, exact)):
            experts[layer, h], tiers[layer, h] = e, ids[t]
    return experts.reshape(shape), tiers.reshape(shape)


def _pairs_within_bound(rels, bound: float, work, costs, exact: int) -> list:
    """The selection of `routes_from_fidelity_tiers` on ONE layer: `rels[t][h]` the three float32 rel of tier index t and head h
    as Python floats (column 0 coreset, 1 sliding tile, 2 full attention in that tier); per head the (tier index, expert) of
    the cheapest candidate with rel <= bound, (T-1, 0) where none qualifies.  `routes_within_cost_share` calls it too, so the
    two rules share one selection."""
    T = len(rels)
    pairs = []
    for h in range(len(rels[0])):
        best = None  # (cost, tier index, -expert): the smallest wins
        for t in range(T):
            for e in (0, 1, 2):
                rel = 0.0 if (e == 0 and t == exact) else rels[t][h][2 if e == 0 else _COLUMN_OF_EXPERT[e]]
                if rel <= bound:
                    key = (float(work[e]) * costs[t], t, -e)
                    best = key if best is None or key < best else best
        pairs.append((T - 1, 0) if best is None else (best[1], -best[2]))
    return pairs


class CostShareRoutes(NamedTuple):
    """`routes_within_cost_share`: per layer, on the CPU"""
    experts: torch.Tensor      # (..., H) int64: 0 full attention, 1 coreset, 2 sliding tile
    tiers: torch.Tensor        # (..., H) int64: GLOBAL precision tier ids (0 native, 1 fp8pv, 2 i8pv)
    level: torch.Tensor        # (...,) float32: r*, the error the budget bought
    cost_share: torch.Tensor   # (...,) float32: the routed layer's cost over all heads on full attention in the last tier


def routes_within_cost_share(fids, max_cost_share: float, geometry: Optional[Geometry] = None, text_valid: int = 0, *,
                             tier_cost: Optional[Mapping] = None) -> CostShareRoutes:
    """Per head the expert AND the precision tier to launch it in, by a COST budget: spend at most `max_cost_share` of what the
    layer costs with every head on full attention in the last tier, on any expert in any tier, where it hurts least.  `fids`,
    `geometry`, `text_valid`, `tier_cost`, the candidates (t, e), their rel (float32) and their cost c[t][e] = work[e] *
    tier_cost[t] (one rounded double product) are `routes_from_fidelity_tiers`', on which this function is written.
    Definitions.  state(r), for a float32 r >= 0: the table `routes_from_fidelity_tiers` gives at the bound r -- its own
    selection (`_pairs_within_bound`, one body for both rules) on rel formed as the device forms it, the divide and the square
    root each correctly rounded in float32 (`_rel_error_float32`), so that a level and the rel it came from are one number.
    cost(table) = the sum over (t, e), t-major, of n[t][e] * c[t][e] from the integer counts, every product and sum rounded
    on its own, an empty list adding nothing.  budget = max_cost_share * (H * c[T-1][0]), two rounded products in that order;
    a table is within it unless cost > budget (equality is within).  The levels are 0 and every finite rel of a candidate.
    The rule.  r* is the smallest level whose state is within the budget; where no level is, the candidates ran out: r* is
    the largest level, the result is state(r*) and `cost_share` > `max_cost_share` shows it.  With r* == 0 the result is
    state(0).  Else start from state(r-), r- the largest level below r*, and move the heads whose pair in state(r*) is
    STRICTLY cheaper than their pair in state(r-) to it, in ascending head id, one at a time, until the cost is within the
    budget: no head's error is raised for nothing, and an equal cost moves no head.  `level` = r*: every head that had a
    qualifying candidate is within it on the sampled rows (a (T-1, 0) fallback head without a `native` tier is not covered,
    as in the bound rule).
    The result minimises the largest per-head rel over all assignments within the budget: an assignment whose largest rel
    is below r* costs at least cost(state(r-)), which is over the budget.
    How r* and the partial step are FOUND is part of the definition, so that the device can be held to it with `==` on every
    record: r* by bisection over the float32 pattern of r (0 .. the pattern of +inf, the midpoint lo + (hi - lo) // 2), the
    partial step by bisection over the head index m in 0 .. H (the heads below m move).  Both are the searches above wherever
    the cost of a state does not grow with r, and that is the case whenever no head leaves the (T-1, 0) fallback for a DEARER
    pair: always with a `native` tier (a head is never without a candidate), and without one whenever full attention in the
    last tier is the dearest pair of the call -- the order "cheapest tier first" with full attention the dearest expert.  In
    another order the bisection still ends on a level whose state is within the budget (or reports that the candidates ran
    out), but a smaller such level may exist.
    With one tier this is NOT `routes_from_fidelity(max_flops_share=...)`: that rule gives a head ONE candidate, its
    smaller-rel sparse expert; this one lets a head step down twice (coreset, then sliding tile).  Neither rule changes.
    ValueError for a share that is zero, negative or NaN, and for what `ops.tier_plan` refuses.
    This function is the definition: `ops.route_budget_tiers` (vorta_route_budget_tiers) applies it on the device."""
    import numpy as np
    from ..ops import DEFAULT_ROUTE_WORK, tier_plan
    if max_cost_share is None or isinstance(max_cost_share, (bool, str)) or not float(max_cost_share) > 0:
        raise ValueError(f"routes_within_cost_share: max_cost_share={max_cost_share!r} (a positive share)")
    share = float(max_cost_share)
    ids, costs, exact = tier_plan(fids, tier_cost)
    work = DEFAULT_ROUTE_WORK if geometry is None else expert_work(geometry, text_valid)
    T = len(ids)
    c = [[float(work[e]) * costs[t] for e in range(3)] for t in range(T)]
    records = list(fids.values())
    shape = tuple(records[0].sq_err.shape[:-1])
    H = shape[-1]
    sq_ref = records[0].sq_ref.detach().cpu().float().reshape(-1, H)
    sq_errs = [f.sq_err.detach().cpu().float().reshape(-1, H, 3) for f in records]
    N = sq_ref.shape[0]
    dense = H * c[T - 1][0]
    budget = share * dense

    def counts(experts, tiers):
        n = [[0, 0, 0] for _ in range(T)]
        for e, t in zip(experts, tiers):
            n[t][e] += 1
        return n

    def cost(n):  # from the integer counts, t-major: the order of the moves cannot change the bits
        total = 0.0
        for t in range(T):
            for e in range(3):
                if n[t][e]:
                    total = total + n[t][e] * c[t][e]
        return total

    out_e = torch.zeros((N, H), dtype=torch.int64)
    out_t = torch.zeros((N, H), dtype=torch.int64)
    level = torch.zeros(N, dtype=torch.float32)
    cost_share = torch.zeros(N, dtype=torch.float32)
    for layer in range(N):
        # rel with BOTH operations correctly rounded in float32, as the device forms it: the levels and the states come from
        # the same numbers, so a head whose rel IS a level qualifies at it (a math library's square root may be an ulp off)
        rels = []  # [t][h] = the three columns
        for t in range(T):
            cols = [_rel_error_float32(sq_errs[t][layer][:, col], sq_ref[layer]) for col in range(3)]
            rels.append([[cols[0][h], cols[1][h], cols[2][h]] for h in range(H)])

        def state(r):  # `routes_from_fidelity_tiers`' selection at the bound r: (experts, tier indices)
            pairs = _pairs_within_bound(rels, r, work, costs, exact)
            return [e for _, e in pairs], [t for t, _ in pairs]

        found = {0.0}
        for t in range(T):
            for col in range(3):
                if col == 2 and t == exact:
                    continue  # (the exact tier's full attention is the reference: the level 0)
                found.update(rels[t][h][col] + 0.0 for h in range(H) if math.isfinite(rels[t][h][col]))
        levels = sorted(found)
        states = {}  # level index -> (experts, tiers, within the budget): state(r) is the state of the largest level <= r

        def at(index):
            if index not in states:
                experts, tiers = state(levels[index])
                states[index] = (experts, tiers, not cost(counts(experts, tiers)) > budget)
            return states[index]

        # r*: bisection over the float32 PATTERN of r (non-negative floats order like their patterns), 0 .. the pattern of
        # +inf, which stands for "no level is within"
        lo, hi = 0, _INF_PATTERN
        while lo < hi:
            mid = lo + (hi - lo) // 2
            r = float(np.array(mid, dtype=np.uint32).view(np.float32))
            if at(bisect.bisect_right(levels, r) - 1)[2]:
                hi = mid
            else:
                lo = mid + 1
        if hi == _INF_PATTERN:  # the candidates ran out
            star = len(levels) - 1
            experts, tiers, _ = at(star)
        else:
            star = bisect.bisect_right(levels, float(np.array(hi, dtype=np.uint32).view(np.float32))) - 1
            experts, tiers, _ = at(max(star - 1, 0))
            to_e, to_t, _ = at(star)
            moves = [h for h in range(H) if c[to_t[h]][to_e[h]] < c[tiers[h]][experts[h]]]  # (none at r* == 0)

            def moved(m):  # the heads below m that get strictly cheaper moved to their pair in state(r*)
                e, t = list(experts), list(tiers)
                for h in moves:
                    if h < m:
                        e[h], t[h] = to_e[h], to_t[h]
                return e, t

            # the partial step: bisection over the head index, 0 (state(r-), over the budget) .. H (every such head moved)
            m_lo, m_hi = 0, H
            while m_hi - m_lo > 1:
                mid = (m_lo + m_hi) // 2
                if cost(counts(*moved(mid))) > budget:
                    m_lo = mid
                else:
                    m_hi = mid
            experts, tiers = moved(m_hi)
        experts, tiers, r_star = list(experts), list(tiers), levels[star]
        out_e[layer] = torch.tensor(experts)
        out_t[layer] = torch.tensor([ids[t] for t in tiers])
        level[layer] = float(np.float32(r_star))
        cost_share[layer] = float(np.float32(cost(counts(experts, tiers)) / dense))
    return CostShareRoutes(out_e.reshape(shape), out_t.reshape(shape), level.reshape(shape[:-1]), cost_share.reshape(shape[:-1]))


class RepairedRoutes(NamedTuple):
    """`repair_routes`: the tables of one layer after the rule, all int64 on the CPU (rel float32)"""
    expert_of_head: torch.Tensor   # (H,): as given, a repaired head 0
    tier_of_head: torch.Tensor     # (H,) caller's tier indices: as given (zeros for None), a repaired head `exact_tier`
    lists: torch.Tensor            # (n_tiers, 3, H): ascending heads per (tier, expert); -1 at and past the count
    counts: torch.Tensor           # (n_tiers, 3)
    repair_list: torch.Tensor      # (H,): ascending heads repaired by THIS call; -1 at and past the count
    repair_count: int
    state_of_head: torch.Tensor    # (H,): 0 not checked, 1 kept, 2 repaired
    rel: torch.Tensor              # (H,) float32: the error as checked; NaN for a head that was not checked


REPAIR_NOT_CHECKED, REPAIR_KEPT, REPAIR_REPAIRED = 0, 1, 2


def _rel_error_float32(sq_err: torch.Tensor, sq_ref: torch.Tensor) -> list:
    """`SampledFidelity.rel_error` of CPU float32 (H,) tensors as Python floats, with BOTH operations correctly rounded in
    float32 and the zero rules of `csrc/route_rel_error.h`.  Element by element in numpy float32, whose divide and square root
    are the IEEE ones: a vectorised `torch.sqrt` on the host may be a math library's, good to an ulp and not to the bit, and a
    head whose error sits on the bound must fall on the same side on the host and on the device."""
    import numpy as np
    err, ref = sq_err.numpy().astype(np.float32), sq_ref.numpy().astype(np.float32)
    with np.errstate(all="ignore"):
        rel = np.sqrt(np.divide(err, ref, dtype=np.float32), dtype=np.float32)
    zero = ref == 0
    rel = np.where(zero & (err == 0), np.float32(0), rel)
    rel = np.where(zero & (err > 0), np.float32(np.inf), rel)
    return [float(x) for x in rel]


def repair_routes(expert_of_head, tier_of_head, n_tiers: int, exact_tier: int, sq_ref, sq_err,
                  repair_above: float) -> RepairedRoutes:
    """Which heads of one layer, AS LAUNCHED, are further than `repair_above` from dense attention on the sampled rows, and the
    routes without them.  `expert_of_head` (H,): 0 / 1 / 2, -1 = no list names the head; `tier_of_head` (H,): the caller's tier
    index of every head, None for one tier; `exact_tier`: the index of the tier whose full attention is the reference
    (`native`); `sq_ref`, `sq_err` (H,): the fields of the `ops.SampledFidelity` the launches were verified by.
    The rule, per head.  A head with expert -1, or already at (expert 0, `exact_tier`), is NOT CHECKED and kept as it is.
    Every other head is checked: rel = `SampledFidelity.rel_error` in float32 (a correctly rounded divide and square root;
    sq_ref == 0 gives 0 where sq_err == 0 and inf where sq_err > 0); it is KEPT iff rel <= float32(repair_above).  NaN meets
    no bound: a NaN record, and a head the measurement left out, are repaired.  A head that is not kept is REPAIRED: it
    becomes (expert 0, `exact_tier`).  Applied again to its own output with the same record the rule repairs nothing.
    ValueError for n_tiers outside 1..3, exact_tier outside 0..n_tiers-1, a NaN or negative bound, 0 or more than 1024
    heads, tables of other shapes, an expert outside -1..2, a tier outside 0..n_tiers-1 and a missing `tier_of_head` with
    more than one tier.
    This function is the definition: `ops.route_repair` (vorta_route_repair) applies it on the device, in place."""
    n_tiers, exact_tier = int(n_tiers), int(exact_tier)
    if not 1 <= n_tiers <= 3:
        raise ValueError(f"repair_routes: n_tiers={n_tiers} (1 to 3)")
    if not 0 <= exact_tier < n_tiers:
        raise ValueError(f"repair_routes: exact_tier={exact_tier} (0 to n_tiers-1 = {n_tiers - 1})")
    if repair_above is None or not float(repair_above) >= 0:
        raise ValueError(f"repair_routes: repair_above={repair_above} (a bound >= 0)")
    experts = torch.as_tensor(expert_of_head).detach().cpu()
    H = experts.numel()
    if experts.dim() != 1 or experts.is_floating_point() or not 1 <= H <= 1024:
        raise ValueError("repair_routes: expert_of_head: an integer table (H,) of 1 to 1024 heads (the tables of ONE layer)")
    if tier_of_head is None:
        if n_tiers != 1:
            raise ValueError(f"repair_routes: tier_of_head=None with n_tiers={n_tiers}: only one tier goes without the table")
        tiers = torch.zeros(H, dtype=torch.int64)
    else:
        tiers = torch.as_tensor(tier_of_head).detach().cpu()
        if tiers.is_floating_point() or tuple(tiers.shape) != (H,):
            raise ValueError(f"repair_routes: tier_of_head: an integer table ({H},), got {tuple(tiers.shape)} {tiers.dtype}")
    experts, tiers = experts.long().clone(), tiers.long().clone()
    if bool(((experts < -1) | (experts > 2)).any()):
        raise ValueError("repair_routes: expert ids are -1 (no list), 0 (full), 1 (coreset), 2 (sliding tile)")
    if bool(((tiers < 0) | (tiers >= n_tiers)).any()):
        raise ValueError(f"repair_routes: tier indices are 0 to n_tiers-1 = {n_tiers - 1}")
    ref, err = (torch.as_tensor(x).detach().cpu().float() for x in (sq_ref, sq_err))
    if tuple(ref.shape) != (H,) or tuple(err.shape) != (H,):
        raise ValueError(f"repair_routes: sq_ref and sq_err ({H},), got {tuple(ref.shape)} and {tuple(err.shape)}")
    bound = float(torch.tensor(float(repair_above), dtype=torch.float32))  # the comparison is float32's
    rel_all = _rel_error_float32(err, ref)
    state = torch.zeros(H, dtype=torch.int64)
    rel = torch.full((H,), float("nan"), dtype=torch.float32)
    repaired = []
    for h in range(H):
        e, t = int(experts[h]), int(tiers[h])
        if e < 0 or (e == 0 and t == exact_tier):
            continue
        rel[h] = rel_all[h]
        if rel_all[h] <= bound:  # (NaN meets no bound)
            state[h] = REPAIR_KEPT
            continue
        state[h] = REPAIR_REPAIRED
        experts[h], tiers[h] = 0, exact_tier
        repaired.append(h)
    lists = torch.full((n_tiers, 3, H), -1, dtype=torch.int64)
    counts = torch.zeros((n_tiers, 3), dtype=torch.int64)
    for h in range(H):
        e, t = int(experts[h]), int(tiers[h])
        if e >= 0:
            lists[t, e, counts[t, e]] = h
            counts[t, e] += 1
    repair_list = torch.full((H,), -1, dtype=torch.int64)
    repair_list[:len(repaired)] = torch.tensor(repaired, dtype=torch.int64)
    return RepairedRoutes(experts, tiers, lists, counts, repair_list, len(repaired), state, rel)


def evaluate_routing(experts_or_scores: torch.Tensor, fid: Union[ExpertFidelity, SampledFidelity], geometry: Geometry,
                     text_valid: int = 0, tau_sparse: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """What a routing costs and what it loses, per layer.  `experts_or_scores`: an integer (L, H) expert table, or floating
    routing scores (L, H, 3) / (L, B, H, 3) (batch item 0; the processors' rule: the first maximum, full attention where
    that score is below `tau_sparse`).  Returns CPU tensors of L entries: `worst_rel_error` and `mean_rel_error` of the
    chosen experts over the heads (a head on full attention contributes 0), `flops_share` = the routed layer's FLOPs over
    the all-dense layer's by `expert_work`, and the table itself as `experts` (L, H).
    With a `SampledFidelity` (`routed_fidelity_of`) a head's error is its MEASURED one, whatever its expert: the routed output
    as run against dense attention, so a full-attention head measured under heads="all" contributes what its precision
    costs; a full-attention head that was not measured contributes 0, a sparse head that was not measured NaN.  The table
    must then be the routes the record was launched with (its `expert`), wherever the record knows them."""
    t = experts_or_scores.detach().cpu()
    if t.is_floating_point():
        if t.dim() == 4:
            t = t[:, 0]
        t = t.float()
        best = t.max(dim=-1).values
        experts = torch.where(t == best.unsqueeze(-1), torch.arange(t.shape[-1]), t.shape[-1]).min(dim=-1).values  # first maximum
        if tau_sparse is not None:
            experts = torch.where(best < float(tau_sparse), torch.zeros_like(experts), experts)
    else:
        experts = t.long()
    rel = fid.rel_error().detach().cpu()
    sampled = isinstance(fid, SampledFidelity)
    if experts.shape != (rel.shape if sampled else rel.shape[:-1]):
        raise ValueError(f"routing table {tuple(experts.shape)} does not match the statistics "
                         f"{tuple(rel.shape if sampled else rel.shape[:-1])}")
    if bool(((experts < 0) | (experts > 2)).any()):
        raise ValueError("expert ids are 0 (full), 1 (coreset), 2 (sliding tile)")
    if sampled:
        launched = None if fid.expert is None else fid.expert.detach().cpu().long()
        if launched is not None and bool(((launched >= 0) & (launched != experts)).any()):
            raise ValueError("the routing table differs from the routes the sampled statistics were launched with (fid.expert)")
        chosen = torch.where(torch.isnan(rel) & (experts == 0), torch.zeros_like(rel), rel)
    else:
        chosen = torch.zeros(experts.shape, dtype=rel.dtype)
        for e, col in _COLUMN_OF_EXPERT.items():
            chosen = torch.where(experts == e, rel[..., col], chosen)
    work = torch.tensor(expert_work(geometry, text_valid), dtype=torch.float64)
    share = work[experts].sum(-1) / (work[0] * experts.shape[-1])
    return dict(worst_rel_error=chosen.max(dim=-1).values, mean_rel_error=chosen.mean(dim=-1), flops_share=share.float(),
                experts=experts)
