"""Shared machinery of the model / pipeline patches (vorta/patch/modeling_*.py, pipeline_*.py).

The reference threads three things through re-stated copies of the diffusers forwards: the pure timestep
embedding into every block's Router (modeling_hunyuan.py:206,350,491,555; modeling_wan.py:77,127,215), the
`self_attention_kwargs` into every self-attention call (modeling_hunyuan.py:492-499; modeling_wan.py:131-137), and the
routing scores back out (modeling_hunyuan.py:296-297,441-449).  This build keeps the stock diffusers forwards and
attaches to them with module hooks instead:

  * a forward hook on the timestep embedder captures the embedding once per forward and computes the routes of
    ALL layers in one call (vorta_route_plan: 2 launches per step instead of ~5 per layer);
  * every block's attention processor is a `BoundProcessor` that adds its layer's routes + the step's keyword
    set to the stock call `proc(attn, hidden_states, encoder_hidden_states, attention_mask, rotary)`;
  * a pre-hook / hook pair on the transformer accepts and strips the extra keywords of the reference's routed
    forward (`self_attention_kwargs`, `return_routing_scores`, `return_losses`, ...) and shapes the output like
    modeling_hunyuan.py:441-449.

Nothing is patched at class level, so two differently patched models can live in one process (the reference
overwrites `Class.forward`, SURVEY.md §8b "not re-entrant").

Training (`train_router=True`, processors built with `differentiable=True`, grad mode on): the scores come from
`Router.forward_autograd` and carry a graph to the router weights (`RoutePlan.compute_autograd`); what the blocks of one
forward need lives in that forward's `ForwardState`, which a block recomputed under gradient checkpointing finds again
(`StepContext.state_for`); `original_attention(model)` is the dense teacher pass, `routing_scores_of(model)` hands the
caller's losses the scores.  Under sequence parallelism the same forward trains frame-sharded or, inside
`token_sharded(model)`, token-sharded; `all_reduce_router_grads(model)` sums the ranks' shares of the router gradients
afterwards.  `expert_fidelity(model)` / `fidelity_of(model)` (patch/fidelity.py) measure how far every head's
sparse experts are from full attention in such a forward.
"""
from __future__ import annotations

import contextlib
import inspect
import weakref
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from .. import ops
from ..routed import HeadRouting
from ..ulysses import SP_STATE

_EXTRA_FORWARD_KEYS = ("self_attention_kwargs", "return_losses", "reture_hidden_layer_distill_loss",
                       "return_routing_scores")


class RoutePlan:
    """Routes of every layer for the current denoising step, resident on the device.

    The router input is the same timestep embedding for all blocks, so one `vorta_route_plan` call at the top of
    the transformer forward replaces the per-block Router module calls + top-k + nonzero of the reference.  Buffers
    are allocated once (fixed addresses: a captured hipGraph of the step replays against new routes)."""

    def __init__(self, routers: Sequence[nn.Module]):
        self.routers = list(routers)
        self.heads = self.routers[0].heads
        self.num_experts = self.routers[0].num_experts
        if any(r.heads != self.heads or r.num_experts != self.num_experts for r in self.routers):
            raise ValueError("all routers of a model must have the same number of heads and experts")
        self._key = None
        self._w = self._b = None
        self._out = None
        self._experts_host: Optional[List[List[int]]] = None
        self.tau = 0.0

    def __len__(self):
        return len(self.routers)

    def _stacked(self, device, dtype):
        params = [(r.linear.weight, r.linear.bias) for r in self.routers]
        key = (str(device), dtype) + tuple((w.data_ptr(), w._version, b.data_ptr(), b._version) for w, b in params)
        if key != self._key:  # first use, or a checkpoint was loaded / the model was moved
            self._w = torch.stack([w.detach().to(device=device, dtype=dtype) for w, _ in params]).contiguous()
            self._b = torch.stack([b.detach().to(device=device, dtype=dtype) for _, b in params]).contiguous()
            self._key = key
            self._out = None
        return self._w, self._b

    @torch.no_grad()
    def compute(self, temb: torch.Tensor, tau: float) -> None:
        """temb: (B, E) pure timestep embedding.  Runs the routers in their own dtype (bf16 in the reference's
        scripts, scripts/hunyuan/inference.py:117) -- the scores are rounded exactly like Router.forward."""
        dtype = self.routers[0].linear.weight.dtype
        if dtype not in (torch.bfloat16, torch.float16):
            dtype = torch.bfloat16
        w, b = self._stacked(temb.device, dtype)
        x = temb.detach().to(dtype)
        if self._out is not None and self._out[0].shape[1] != x.shape[0]:
            self._out = None
        if self._out is None:  # first step (or new shapes): allocate the four buffers
            self._out = ops.route_plan(x, w, b, self.heads, float(tau), self.num_experts)
        else:  # the same buffers at the same addresses, through the custom op (traceable; hipGraph replay reads them)
            from .. import torch_ops  # noqa: F401
            torch.ops.vorta.route_plan_(x, w, b, self.heads, float(tau), self.num_experts, *self._out)
        self._experts_host = None
        self.tau = float(tau)

    def trainable(self) -> bool:
        return any(p.requires_grad for r in self.routers for p in r.parameters())

    def compute_autograd(self, temb: torch.Tensor) -> torch.Tensor:
        """(L, B, H, E) scores with a graph to every router's weights and to `temb` (not detached: a trainable timestep
        embedder gets its gradient): `Router.forward_autograd` layer by layer, its roundings and its bits.  The hard
        dispatch lists are not computed: the soft-mixture processors do not read them."""
        return torch.stack([r.forward_autograd(temb) for r in self.routers])

    @property
    def ready(self) -> bool:
        return self._out is not None

    def all_scores(self) -> torch.Tensor:
        return self._out[0]  # (L, B, H, E)

    def scores(self, layer: int) -> torch.Tensor:
        return self._out[0][layer]  # (B, H, E)

    def routing(self, layer: int) -> HeadRouting:
        return HeadRouting.from_device(self._out[2][layer], self._out[3][layer])

    def experts_host(self, layer: int) -> List[int]:
        """head -> expert of one layer on the host; ONE device read per step for all layers (the sequence-parallel
        head placement needs it; the reference reads torch.nonzero per expert per layer, hunyuan.py:633)."""
        if self._experts_host is None:
            self._experts_host = self._out[1].cpu().tolist()
        return self._experts_host[layer]


@dataclass(eq=False)
class ForwardState:
    """What the attention blocks of ONE forward of a patched model are handed: the keyword set (for Hunyuan with the
    sliding-tile descriptor in it), this forward's scores and the teacher flag.  A block recomputed during `backward()`
    (gradient checkpointing) is handed the same objects again, whatever forwards ran in between."""
    kwargs: Optional[Dict[str, Any]] = None      # self_attention_kwargs of this forward, completed
    teacher: bool = False                        # forward under `original_attention`: dense attention, no route plan
    scores: Optional[torch.Tensor] = None        # (L, B, H, E); with a graph on the training path
    layer_scores: List[torch.Tensor] = field(default_factory=list)  # its per-layer views, made once
    head_routing: bool = False                   # the plan's dispatch lists belong to these scores (inference path)
    fidelity: Optional[Dict[int, Any]] = None    # layer -> ops.ExpertFidelity; a dict only under `expert_fidelity(model)`
    # layer -> [ops.SampledFidelity per batch item]; a dict only under `routed_fidelity(model)`, whose (n_rows, seed, heads)
    # this forward read when it started
    routed_fidelity: Optional[Dict[int, Any]] = None
    measure_routed: Optional[Tuple[int, int, str]] = None
    # layer -> [ops.ExpertFidelity per batch item]; a dict only under `sampled_expert_fidelity(model)`, whose (n_rows, seed)
    # this forward read when it started
    sampled_experts: Optional[Dict[int, Any]] = None
    measure_experts: Optional[Tuple[int, int]] = None
    # inside `fixed_routes(model, table)`: the (L, H) expert table this forward launches, and its per-layer HeadRouting
    fixed_routes: Optional[List[List[int]]] = None
    fixed_routing: Dict[int, HeadRouting] = field(default_factory=dict)
    # `fixed_routes(model, table, precisions=...)`: the (L, H) table of global tier ids, and per layer tier -> HeadRouting
    fixed_precisions: Optional[List[List[int]]] = None
    fixed_tier_routing: Dict[int, Dict[str, HeadRouting]] = field(default_factory=dict)
    # inside `measured_routes(model, ...)`: the context's state (patch/fidelity.py MeasuredRoutes) and whether THIS forward
    # measures (forwards 0, k, 2k, ... of the context) or launches the lists the latest measuring forward stored
    measured_routes: Any = None
    measures_routes: bool = False
    # inside `measured_routes(..., repair_above=b)` / `fixed_routes(..., repair_above=b)`: the context's RouteRepair
    # (patch/fidelity.py): every routed call of this forward verifies what it launched and repairs the heads over the bound
    route_repair: Any = None
    token_shard: bool = False                    # sequence parallel: this forward got the WHOLE latent and cuts its tokens itself


class _KeepState(torch.autograd.Function):
    """Identity on the model output whose graph node owns the forward's `ForwardState`: the state lives exactly as long
    as something can still run a backward (and so a recompute) through this forward, and not a moment longer."""

    @staticmethod
    def forward(ctx, x, state):
        ctx.state = state
        return x.view_as(x)

    @staticmethod
    def backward(ctx, grad):
        return grad, None


def all_reduce_sp(tensors: Sequence[torch.Tensor], average: bool = False) -> List[torch.Tensor]:
    """ONE all-reduce over the sequence-parallel group of `tensors` taken together: summed in float32 (one rounding back to
    each tensor's dtype), or averaged.  Returns new tensors; a gloo group reduces host copies, as `gather_fidelity` gathers
    them.  A collective: every rank calls it with tensors of the same shapes in the same order."""
    import torch.distributed as dist
    flat = torch.cat([t.detach().reshape(-1).float() for t in tensors])
    staged = dist.get_backend(SP_STATE.group) == "gloo"
    buf = flat.cpu() if staged else flat
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=SP_STATE.group)
    if average:
        buf = buf / SP_STATE.sp_size
    buf = buf.to(flat.device)
    out, at = [], 0
    for t in tensors:
        out.append(buf[at:at + t.numel()].view(t.shape).to(t.dtype))
        at += t.numel()
    return out


class _SumOverRanks(torch.autograd.Function):
    """Identity on the text rows a joint-attention block (Hunyuan) hands its processor under sequence parallelism, whose
    backward sums the cotangent over the group.  The exchange's two text conventions do not compose on their own
    (ulysses/autograd.py): the scatter's backward leaves a rank the text-row gradient of ITS OWN heads (partial: the ranks'
    sum is the gradient), the gather's backward takes the rank's own heads out of a cotangent it assumes REPLICATED (every
    rank sees the same loss on the text rows).  One layer alone satisfies both; in a stack, layer l + 1 hands layer l a
    partial cotangent through the text stream and the other ranks' shares of a head's text rows would be dropped.  Summed
    here, the text stream between two layers carries the whole cotangent on every rank, which is what the gather reads."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, grad):
        return all_reduce_sp([grad])[0]


def _rotary_key(rotary) -> Optional[torch.Tensor]:
    if isinstance(rotary, (tuple, list)):
        rotary = rotary[0] if rotary else None
    return rotary if isinstance(rotary, torch.Tensor) else None


@dataclass
class StepContext:
    """Per-model state shared by the hooks and the bound processors.

    Per-forward state: `current` is the `ForwardState` of the running forward (strong, from the model's pre hook to its
    post hook).  Every bound processor call inside it also files the state under the rotary table it was handed --
    `records`: id(table) -> (weak table, weak states).  A NON-REENTRANT checkpoint replays a block with the very argument
    tensors of its forward, so the recomputed block finds its own forward's state by that table, after the post hook has
    run and whichever forwards (the teacher's, the next step's) ran since.  The state itself is owned by the graph of the
    model output (`_KeepState`), so it is released with the last tensor that could run that backward; nothing here holds
    it strongly and there is no cycle through the model.  A reentrant checkpoint replays with detached copies of the
    arguments, finds no record and is refused with an error that says so."""
    plan: Optional[RoutePlan] = None
    current: Optional[ForwardState] = None
    records: Dict[int, Tuple[Any, List[Any]]] = field(default_factory=dict)
    teacher: bool = False                             # inside `original_attention(model)`
    differentiable: bool = False                      # the bound processors were built with differentiable=True
    student: Any = None                               # weak reference to the latest student forward's state
    student_scores: Optional[torch.Tensor] = None     # its scores, detached (what outlives the graph)
    default_kwargs: Optional[Dict[str, Any]] = None   # set by the pipeline call; used when the forward gets none
    return_routing_scores: bool = False
    default_return_routing_scores: bool = False
    collected: List[Any] = field(default_factory=list)  # per-step score lists gathered for the pipeline call
    step_token: Any = None       # callable -> object identifying the running denoising step (pipeline call)
    last_token: Any = None
    descriptor_cache: Dict[Any, Any] = field(default_factory=dict)
    forwards: int = 0
    needs_tau: bool = True       # hard top-1 dispatch (Eval processors); False for the soft mixture (Train)
    # pipeline calls and `token_sharded(model)`: the model gets the WHOLE latent and shards its token sequence itself (read
    # once per forward, into `ForwardState.token_shard`)
    sp_token_shard: bool = False
    sp_coherent: bool = False     # this call's / context's ranks were seen to hold the same tokens (install_token_shard)
    measure_fidelity: bool = False  # inside `expert_fidelity(model)` (patch/fidelity.py)
    fidelity: Optional[Dict[int, Any]] = None  # the statistics of the latest forward that measured (what `fidelity_of` reads)
    measure_routed: Optional[Tuple[int, int, str]] = None  # inside `routed_fidelity(model)`: (n_rows, seed, heads)
    routed_fidelity: Optional[Dict[int, Any]] = None  # the latest measured routed forward's records (`routed_fidelity_of`)
    measure_experts: Optional[Tuple[int, int]] = None  # inside `sampled_expert_fidelity(model)`: (n_rows, seed)
    sampled_experts: Optional[Dict[int, Any]] = None  # the latest such forward's records (`sampled_expert_fidelity_of`)
    fixed_routes: Optional[List[List[int]]] = None  # inside `fixed_routes(model, table)`: the (L, H) expert table
    fixed_precisions: Optional[List[List[int]]] = None  # ... and with `precisions=`: the (L, H) table of global tier ids
    measured_routes: Any = None  # inside `measured_routes(model, ...)`: its MeasuredRoutes (rule, forward count, stored lists)
    latest_measured_routes: Any = None  # that of the latest context left (what `measured_routes_of` reads outside one)
    route_repair: Any = None  # inside a context with `repair_above`: its RouteRepair (bound, sample, per-layer tables and records)
    latest_route_repair: Any = None  # that of the latest context left (what `repaired_routes_of` reads outside one)

    def state_for(self, rotary) -> Optional[ForwardState]:
        """the state of the forward a processor call belongs to: the running forward's (in grad mode filed under `rotary`
        for a later recompute), else the one filed under `rotary` by the forward that made the table; None when there is
        neither"""
        key = _rotary_key(rotary)
        hit = self.records.get(id(key)) if key is not None else None
        if hit is not None and hit[0]() is not key:  # the address of a table that is gone
            hit = None
        state = self.current
        if state is not None:
            if key is not None and torch.is_grad_enabled() and (hit is None or all(s() is not state for s in hit[1])):
                # a rope that caches its table hands one object to many forwards: keep those whose state is still alive
                alive = [s for s in hit[1] if s() is not None] if hit is not None else []
                records, kid = self.records, id(key)
                wkey = hit[0] if hit is not None else weakref.ref(key, lambda _, r=records, k=kid: r.pop(k, None))
                records[kid] = (wkey, alive + [weakref.ref(state)])
            return state
        alive = [x for x in (s() for s in hit[1]) if x is not None] if hit is not None else []
        if len(alive) > 1:
            raise RuntimeError("a block is recomputed with a rotary table that two forwards with live graphs share: the "
                               "per-forward state is filed under that table and cannot tell them apart")
        return alive[0] if alive else None

    def token_shard_of(self, args=(), kwargs=None) -> bool:
        """token-shard mode of the forward a hook call belongs to: the running forward's; for a module recomputed later by
        a non-reentrant checkpoint, that of the forward on record for a rotary table among its arguments; with neither (a
        model without the routed forward protocol, a module that is handed no table) the flag as it stands"""
        state = self.current
        if state is None and self.records:
            for v in tuple(args) + tuple((kwargs or {}).values()):
                key = _rotary_key(v)
                if key is not None and id(key) in self.records:
                    state = self.state_for(v)
                    if state is not None:
                        break
        return state.token_shard if state is not None else self.sp_token_shard


class BoundProcessor:
    """Adapter between the stock diffusers call `processor(attn, hidden_states, encoder_hidden_states=...,
    attention_mask=..., image_rotary_emb|rotary_emb=...)` and the routed processors' keyword set
    (hunyuan.py:521-539, wan.py:308-328)."""

    def __init__(self, inner, ctx: StepContext, layer: int, rotary_name: str, dense=None, joint_text: bool = False):
        self.inner = inner
        self.dense = dense  # plain dense processor serving `use_original_attn=True` (the teacher path)
        self.joint_text = joint_text  # the text rows attend with the video rows and flow on to the next block (Hunyuan)
        self.ctx = ctx
        self.layer = layer
        self.rotary_name = rotary_name
        params = inspect.signature(inner.__call__).parameters
        self._accepted = set(params)
        # the processor's own default, for a caller whose kwargs leave `latent_shape` to it (the measured path sizes its sample)
        self._default_latent = params["latent_shape"].default if "latent_shape" in params else None

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, image_rotary_emb=None,
                 rotary_emb=None, use_original_attn: bool = False):
        rotary = image_rotary_emb if self.rotary_name == "image_rotary_emb" else rotary_emb
        ctx = self.ctx
        state = ctx.state_for(rotary)
        if state is None:
            raise RuntimeError("this attention block runs outside a forward of its patched transformer and no earlier "
                               "forward is on record for its rotary table.  A block recomputed by gradient checkpointing "
                               "finds its forward by the argument tensors it is replayed with: use the non-reentrant "
                               "form (torch.utils.checkpoint.checkpoint(..., use_reentrant=False)), which replays them "
                               "unchanged; the reentrant form replays detached copies and cannot be served")
        if use_original_attn or state.teacher:
            if "use_original_attn" in self._accepted:
                return self.inner(attn, hidden_states, encoder_hidden_states, attention_mask, rotary,
                                  use_original_attn=True)
            return self.dense(attn, hidden_states, encoder_hidden_states, attention_mask, rotary)
        if state.kwargs is None:
            raise ValueError("this transformer was patched with apply_vorta_transformer: pass `self_attention_kwargs` "
                             "(prepare_*_self_attn_kwargs) to its forward, or run it through vorta_pipeline_call")
        if ctx.plan is None or state.scores is None:
            raise RuntimeError("routes of this step are not available: the timestep embedder of the model was not "
                               "called before its first attention block")
        if (self.joint_text and SP_STATE.enabled and torch.is_grad_enabled() and encoder_hidden_states is not None
                and encoder_hidden_states.requires_grad):
            # a training graph through a stack of joint-attention layers: the text stream carries whole cotangents
            encoder_hidden_states = _SumOverRanks.apply(encoder_hidden_states)
        kw = {k: v for k, v in state.kwargs.items() if k in self._accepted}
        kw["routing_score"] = state.layer_scores[self.layer]
        if state.head_routing:
            if "head_routing" in self._accepted:
                kw["head_routing"] = ctx.plan.routing(self.layer)
            if "experts_host" in self._accepted and SP_STATE.enabled:
                kw["experts_host"] = ctx.plan.experts_host(self.layer)
        if "fidelity_rows" in self._accepted:  # a hard-routing (Eval) processor: its sinks take the ROUTED call's statistics
            repair, psink = state.route_repair, None
            if repair is not None:
                # every routed call verifies what it launched on the context's sample and repairs the heads over the bound
                if "repair_above" not in self._accepted:
                    raise ValueError("repair_above: this model's Eval processor takes no `repair_above`")
                if SP_STATE.enabled:
                    raise NotImplementedError("repair_above: verifying and repairing launched routes does not run under "
                                              "sequence parallelism")
                psink = []
                kw["repair_above"], kw["repair_sink"] = repair.bound, psink
                kw["fidelity_rows"] = repair.rows(kw.get("latent_shape", self._default_latent), hidden_states.device)
            if state.fixed_routes is not None and repair is not None:
                # under `fixed_routes(model, table, repair_above=b)`: this layer's rows of the tables as DEVICE tables, placed
                # once per context entry -- the repairs of a forward persist in them until the context exits
                kw.setdefault("tau_sparse", 0.0)
                routes = repair.fixed_tables(self.layer, state.fixed_routes[self.layer],
                                             None if state.fixed_precisions is None else state.fixed_precisions[self.layer],
                                             hidden_states.device)
                if routes.tier_index is None:
                    kw["head_routing"] = HeadRouting.from_device(routes.lists[0], routes.counts[0], routes.expert_ids)
                elif "tier_routing" not in self._accepted:
                    raise ValueError("fixed_routes(precisions=...): this model's Eval processor takes no `tier_routing`")
                else:
                    kw["tier_routing"] = routes
            elif state.fixed_routes is not None:
                # under `fixed_routes(model, table)`: this layer's row of the table, host counts; the plan's routes and
                # `tau_sparse` are not consulted
                if self.layer not in state.fixed_routing:
                    state.fixed_routing[self.layer] = HeadRouting.from_expert_ids(state.fixed_routes[self.layer],
                                                                                  hidden_states.device)
                kw["head_routing"] = state.fixed_routing[self.layer]
                kw.setdefault("tau_sparse", 0.0)
                if state.fixed_precisions is not None:
                    # ... and this layer's row of the tier table: per tier the heads that run in it, host counts
                    if "tier_routing" not in self._accepted:
                        raise ValueError("fixed_routes(precisions=...): this model's Eval processor takes no `tier_routing`")
                    if self.layer not in state.fixed_tier_routing:
                        from ..ops import TIER_NAMES
                        experts, tiers = state.fixed_routes[self.layer], state.fixed_precisions[self.layer]
                        state.fixed_tier_routing[self.layer] = {
                            TIER_NAMES[t]: HeadRouting.from_expert_ids([e if p == t else -1 for e, p in zip(experts, tiers)],
                                                                       hidden_states.device)
                            for t in sorted(set(tiers), reverse=True)}
                    kw["tier_routing"] = state.fixed_tier_routing[self.layer]
            rsink = None
            if state.measured_routes is not None:
                # under `measured_routes(model, ...)`: a measuring forward routes this layer by its own measurement and
                # stores the device lists; the forwards between two measurements launch the stored lists, nothing more.  The
                # plan's routes and `tau_sparse` are not consulted
                if "route_rule" not in self._accepted:
                    raise ValueError("measured_routes: this model's Eval processor takes no `route_rule`")
                kw.setdefault("tau_sparse", 0.0)
                if state.measures_routes:
                    rsink = []
                    kw["route_rule"], kw["route_sink"] = state.measured_routes.rule, rsink
                elif state.measured_routes.stores_tiers(self.layer):
                    if "tier_routing" not in self._accepted:
                        raise ValueError("measured_routes(covers_precision=True): this model's Eval processor takes no `tier_routing`")
                    # (with a repair: the stored joint tables themselves, which the call rewrites in place)
                    kw["tier_routing"] = (state.measured_routes.stored_tier_routing(self.layer) if repair is None
                                          else state.measured_routes.stored_repairable(self.layer))
                else:
                    kw["head_routing"] = state.measured_routes.stored_routing(self.layer)  # (raises where there is none)
            if state.routed_fidelity is None and state.sampled_experts is None:
                out = self.inner(attn, hidden_states, encoder_hidden_states, attention_mask, rotary, **kw)
                if rsink:  # (a cross-attention call measures nothing)
                    state.measured_routes.file(self.layer, rsink)
                if psink:
                    repair.file(self.layer, psink[0])
                return out
            # under `routed_fidelity(model)` / `sampled_expert_fidelity(model)`: the sample is fixed per (S, n, seed) -- one
            # cached table, no host work per layer; the two share it
            from ..routed import sample_rows
            n_rows, seed = (state.measure_routed or state.measure_experts)[:2]
            S = 1
            for x in kw.get("latent_shape", self._default_latent):
                S *= int(x)
            kw["fidelity_rows"] = sample_rows(S, min(n_rows, S), seed, hidden_states.device)
            sink = esink = None
            if state.routed_fidelity is not None:
                kw["fidelity"] = sink = []
                kw["fidelity_heads"] = state.measure_routed[2]
            if state.sampled_experts is not None:
                if "expert_fidelity" not in self._accepted:
                    raise ValueError("sampled_expert_fidelity: this model's Eval processor takes no `expert_fidelity` sink")
                kw["expert_fidelity"] = esink = []
            out = self.inner(attn, hidden_states, encoder_hidden_states, attention_mask, rotary, **kw)
            if sink:  # (a cross-attention call measures nothing)
                state.routed_fidelity[self.layer] = sink
            if esink:
                state.sampled_experts[self.layer] = esink
            if rsink:
                state.measured_routes.file(self.layer, rsink)
            if psink:
                repair.file(self.layer, psink[0])
            return out
        if state.fidelity is None or "fidelity" not in self._accepted:
            return self.inner(attn, hidden_states, encoder_hidden_states, attention_mask, rotary, **kw)
        kw["fidelity"] = sink = []  # under `expert_fidelity(model)`: the soft mixture's statistics, filed under this layer
        out = self.inner(attn, hidden_states, encoder_hidden_states, attention_mask, rotary, **kw)
        if sink:  # (a cross-attention call measures nothing)
            state.fidelity[self.layer] = sink[-1]
        return out


def set_processor(attn: nn.Module, processor) -> None:
    if hasattr(attn, "set_processor"):
        attn.set_processor(processor)
    else:
        attn.processor = processor


def clear_hooks(model: nn.Module) -> None:
    for h in getattr(model, "_vorta_hooks", []):
        h.remove()
    model._vorta_hooks = []


def add_hook(model: nn.Module, handle) -> None:
    model._vorta_hooks.append(handle)


def context_of(model: nn.Module) -> StepContext:
    ctx = getattr(model, "_vorta_ctx", None)
    if ctx is None:
        ctx = StepContext()
        model._vorta_ctx = ctx
    return ctx


def install_forward_protocol(model: nn.Module, ctx: StepContext, prepare_kwargs=None) -> None:
    """Accept the reference's extra forward keywords on the stock forward and return its output shape:
    `(sample, reg_loss, last_layer_distill_loss, hidden_layer_distill_loss, routing_scores)` when
    `return_dict=False` (modeling_hunyuan.py:441-442, modeling_wan.py:171-172), a RoutedTransformerModelOutput
    otherwise.  `prepare_kwargs(model, args, kwargs, self_attention_kwargs)` may complete the keyword set from
    the forward's own arguments (Hunyuan: the per-prompt sliding-tile descriptor, modeling_hunyuan.py:269-279)."""
    from .outputs import RoutedTransformerModelOutput

    def pre(module, args, kwargs):
        extra = {k: kwargs.pop(k) for k in _EXTRA_FORWARD_KEYS if k in kwargs}
        if extra.get("return_losses") or extra.get("reture_hidden_layer_distill_loss"):
            raise NotImplementedError("router training losses (modeling_hunyuan.py:301-330) are outside the inference "
                                      "hot path of this build")
        sak = extra.get("self_attention_kwargs")
        if sak is None:
            sak = ctx.default_kwargs
        if sak is not None and prepare_kwargs is not None and not ctx.teacher:
            sak = prepare_kwargs(module, args, kwargs, sak)
        token_shard = bool(ctx.sp_token_shard and SP_STATE.enabled)
        if SP_STATE.enabled and not token_shard and sak is not None and sak.get("latent_shape") is not None \
                and int(sak["latent_shape"][0]) % SP_STATE.sp_size:
            raise ValueError(f"a frame-sharded forward needs the {SP_STATE.sp_size} sequence-parallel ranks to divide the "
                             f"latent frame count, which is {int(sak['latent_shape'][0])} (latent_shape "
                             f"{tuple(sak['latent_shape'])}): hand every rank the whole latent inside "
                             "`token_sharded(model)`, or run the pipeline call, which shards tokens")
        measured = None if ctx.teacher else ctx.measured_routes
        measures = measured is not None and measured.begin_forward()  # (the context counts its non-teacher forwards)
        ctx.current = ForwardState(kwargs=sak, teacher=ctx.teacher, measured_routes=measured, measures_routes=measures,
                                   fidelity={} if ctx.measure_fidelity and not ctx.teacher else None,
                                   routed_fidelity={} if ctx.measure_routed is not None and not ctx.teacher else None,
                                   measure_routed=ctx.measure_routed,
                                   sampled_experts={} if ctx.measure_experts is not None and not ctx.teacher else None,
                                   measure_experts=ctx.measure_experts,
                                   fixed_routes=None if ctx.teacher else ctx.fixed_routes,
                                   fixed_precisions=None if ctx.teacher else ctx.fixed_precisions,
                                   route_repair=None if ctx.teacher else ctx.route_repair,
                                   token_shard=token_shard)
        ctx.return_routing_scores = bool(extra.get("return_routing_scores", ctx.default_return_routing_scores))
        ctx.forwards += 1
        return args, kwargs

    def post(module, args, kwargs, output):
        state, ctx.current = ctx.current, None
        if output is None:  # the forward raised (always_call): no later recompute may take its state for the running one
            return None
        scores: List[torch.Tensor] = []
        if state.scores is not None:
            ctx.student, ctx.student_scores = weakref.ref(state), state.scores.detach()
        if state.fidelity:
            ctx.fidelity = state.fidelity  # (small per-head tensors: kept until the next measuring forward)
        if state.routed_fidelity:
            ctx.routed_fidelity = state.routed_fidelity  # (likewise)
        if state.sampled_experts:
            ctx.sampled_experts = state.sampled_experts  # (likewise)
        if ctx.return_routing_scores and state.scores is not None:
            # one device read for all layers (the reference does `.detach().cpu()` per block, modeling_hunyuan.py:297)
            all_scores = state.scores.detach().cpu()
            scores = [all_scores[i] for i in range(all_scores.shape[0])]
            # under the pipeline call only the first (conditional) forward of a step is recorded, as the reference
            # passes return_routing_scores=False to the guidance forward (pipeline_hunyuan.py:424-437)
            token = ctx.step_token() if ctx.step_token is not None else None
            if token is None or token is not ctx.last_token:
                ctx.collected.append(scores)
                ctx.last_token = token  # keeps the object alive, so `is` cannot match a recycled id
        sample = output[0] if isinstance(output, tuple) else output.sample if hasattr(output, "sample") else output
        if torch.is_grad_enabled() and sample.requires_grad:  # a backward may recompute blocks of this forward
            sample = _KeepState.apply(sample, state)
        if isinstance(output, tuple):
            return (sample, None, None, None, scores)
        return RoutedTransformerModelOutput(sample=sample, routing_scores=scores)

    add_hook(model, model.register_forward_pre_hook(pre, with_kwargs=True))
    add_hook(model, model.register_forward_hook(post, with_kwargs=True, always_call=True))


def install_timestep_capture(embedder: nn.Module, model: nn.Module, ctx: StepContext) -> None:
    """Compute the route plan from the output of the timestep embedder -- the reference's `clean_timesteps_emb`
    (modeling_hunyuan.py:627-628,645) / `temb` before `time_proj` (modeling_wan.py:77) -- at its FIRST call in a
    forward (Hunyuan's token_replace variant embeds a second, zero timestep, modeling_hunyuan.py:633-637)."""

    def hook(module, args, output):
        state = ctx.current
        if state is None or state.scores is not None or state.teacher or ctx.plan is None or state.kwargs is None:
            return None
        if torch.is_grad_enabled() and ctx.differentiable and ctx.plan.trainable():
            state.scores = ctx.plan.compute_autograd(output)  # the training path: a graph to the routers
            state.layer_scores = list(state.scores.unbind(0))
            return None
        tau = state.kwargs.get("tau_sparse")
        if tau is None:
            if ctx.needs_tau and state.fixed_routes is None and state.measured_routes is None:
                raise ValueError("self_attention_kwargs has no `tau_sparse` "
                                 "(prepare_*_self_attn_kwargs(..., tau_sparse=...))")
            tau = 0.0  # soft-mixture processors use the scores only; the dispatch lists go unused
        ctx.plan.compute(output, tau)
        state.scores = ctx.plan.all_scores()
        if torch.is_grad_enabled() and ctx.differentiable:
            # frozen routers inside a training graph: a recompute must not read what a later forward wrote into the
            # plan's fixed buffers
            state.scores = state.scores.clone()
        else:
            state.head_routing = True
        state.layer_scores = list(state.scores.unbind(0))
        return None

    add_hook(model, embedder.register_forward_hook(hook))


@contextlib.contextmanager
def original_attention(model: nn.Module):
    """The teacher pass at model level: while active, every forward of `model` (patched with apply_vorta_transformer)
    runs each block's attention dense (`use_original_attn=True`, modeling_hunyuan.py:251-285,426-428) and computes no
    route plan; `self_attention_kwargs` may be left out.  Under torch.no_grad() on the student's inputs this is the
    reference's `ref_hidden_states` stream.  The flag is read once per forward, into that forward's state: a student
    block recomputed later stays a student block, inside this context too."""
    ctx = context_of(model)
    if ctx.plan is None:
        raise ValueError("original_attention: the model was not patched with apply_vorta_transformer")
    previous, ctx.teacher = ctx.teacher, True
    try:
        yield model
    finally:
        ctx.teacher = previous


def routing_scores_of(model: nn.Module) -> torch.Tensor:
    """(L, B, H, E) routing scores of the model's latest student forward, for the caller's losses (the reference's
    `reg_loss` is `mean(scores[..., 0] ** 2)` per layer, modeling_hunyuan.py:301-305).  They carry the graph to the router
    weights when that forward built one (grad mode, trainable routers, differentiable processors) and its output is
    still alive; detached otherwise."""
    ctx = context_of(model)
    if ctx.student_scores is None:
        raise RuntimeError("routing_scores_of: no routed forward of this model has run yet")
    state = ctx.student() if ctx.student is not None else None
    if state is not None and state.scores is not None and state.scores.requires_grad:
        return state.scores
    return ctx.student_scores


def installed_routers(model: nn.Module) -> List[nn.Module]:
    """the Router of every block, in block order, as apply_vorta_transformer installed them"""
    ctx = context_of(model)
    if ctx.plan is None:
        raise ValueError("the model was not patched with apply_vorta_transformer")
    return list(ctx.plan.routers)


def all_reduce_router_grads(model: nn.Module, op: str = "sum") -> None:
    """After a sequence-parallel backward: ONE all-reduce over the sequence-parallel group of the `.grad` of every parameter
    of every Router the patch installed, written back in place.  A rank's backward leaves it the score gradients of its own
    heads and exact zeros elsewhere, so every router holds a partial gradient per rank; `op="sum"` makes
    them the single-process gradient (accumulated in float32, one rounding to the gradient's dtype).  `op="avg"` divides
    that sum by the group size: what an averaging data-parallel wrapper does, right for a loss that is a MEAN over the
    rank's shard.  A term every rank computes identically from replicated values -- the reference's regulariser on
    `routing_scores_of(model)` -- is counted P times by the sum: the caller divides it by P before `backward()`.
    A gloo group reduces host copies.  With sequence parallelism disabled this is a no-op.  A collective: every rank calls
    it, with the same parameter list -- a router parameter without a gradient is an error that names it.
    NOT covered: the gradients of every other parameter and of `encoder_hidden_states`.  They follow the same rule (a
    rank holds its share; parameters applied to replicated values behind a gather, such as the output projection under
    `token_sharded`, hold the whole gradient on every rank) and belong to the training loop."""
    if op not in ("sum", "avg"):
        raise ValueError(f"all_reduce_router_grads: op must be 'sum' or 'avg', got {op!r}")
    routers = installed_routers(model)
    if not SP_STATE.enabled:
        return
    named = [(f"router of block {i}: {n}", p) for i, r in enumerate(routers) for n, p in r.named_parameters()]
    missing = [n for n, p in named if p.grad is None]
    if missing:
        raise RuntimeError("all_reduce_router_grads: no gradient for " + ", ".join(missing) + " on sequence-parallel rank "
                           f"{SP_STATE.group_local_rank}: every rank must reduce the same list (run backward() first; the "
                           "routers are trained with train_router=True)")
    grads = [p.grad for _, p in named]
    with torch.no_grad():
        for g, total in zip(grads, all_reduce_sp(grads, average=op == "avg")):
            g.copy_(total)


@contextlib.contextmanager
def token_sharded(model: nn.Module, check: bool = True):
    """Token-sharded forwards outside the pipeline call, for a training loop: while active and sequence parallelism is
    enabled, every forward of `model` (patched with apply_vorta_transformer) takes the WHOLE latent on every rank and
    shards its token sequence itself, through the hooks the pipeline call uses (`install_token_shard`): any latent whose
    TOKEN count the ranks divide trains, whatever its frame count (Hunyuan-129f: 33 latent frames, 118 800 tokens).
    The flag is read once per forward, into that forward's state, as `original_attention` and `expert_fidelity` are: a
    block recomputed later by a non-reentrant checkpoint sees the mode of its own forward.  `check=True` compares the
    ranks' tokens (`check_rank_coherence`) at the first cut after entering: one read-back per entry, not per forward;
    `check=False` skips it.  The previous mode is restored on exit, after an exception too.  Without sequence parallelism
    the context changes nothing.

    Grad mode.  The cut is a slice and the gather is `ulysses.all_gather`, whose backward hands a rank its own slice of the
    cotangent.  Every rank sees the whole gathered output and computes the SAME loss on it; a rank's gradients -- of the
    router weights, of the latent (non-zero on its own tokens), of every parameter in front of the gather -- are then its
    share, and their sum over the ranks is the single-process gradient (`all_reduce_router_grads` for the routers).  What
    every rank computes identically from replicated values is counted P times by that sum: the caller divides such a term
    by P -- the reference's regulariser on `routing_scores_of(model)` -- and a parameter behind the gather (the output
    projection) holds the whole gradient on every rank.

    Without this context a forward is FRAME-sharded, in grad mode as well: the caller passes its own latent-frame shard,
    `install_sp_rope` supplies the global rotary table, P must divide the frame count, and the loss is the caller's on its
    own output shard."""
    ctx = context_of(model)
    if ctx.plan is None:
        raise ValueError("token_sharded: the model was not patched with apply_vorta_transformer")
    previous = (ctx.sp_token_shard, ctx.sp_coherent)
    ctx.sp_token_shard, ctx.sp_coherent = True, not check
    try:
        yield model
    finally:
        ctx.sp_token_shard, ctx.sp_coherent = previous


def install_sp_rope(rope: nn.Module, model: nn.Module, frame_dim: int = 2) -> None:
    """Sequence parallelism shards the latent frames (pipeline_hunyuan.py:367-369), but rotary positions are global:
    the reference re-states the rope forward with `num_frames * sp_size` (modeling_hunyuan.py:592-620,
    modeling_wan.py:226-252) and the processors narrow the table to their shard (hunyuan.py:89-95).  The stock rope
    only reads the SHAPE and device of its input, so a zero-stride stand-in of the global shape gives the same
    table without touching the module."""

    ctx = context_of(model)

    def pre(module, args):
        if not SP_STATE.enabled or not args or ctx.token_shard_of():  # token shard: the input already is the global latent
            return None
        x = args[0]
        shape = list(x.shape)
        shape[frame_dim] *= SP_STATE.sp_size
        ghost = torch.empty((1,), dtype=x.dtype, device=x.device).as_strided(shape, [0] * len(shape))
        return (ghost,) + tuple(args[1:])

    add_hook(model, rope.register_forward_pre_hook(pre))


COHERENCE_SAMPLE = 64


def coherence_sample_indices(n: int, k: int = COHERENCE_SAMPLE, device=None) -> torch.Tensor:
    """min(k, n) evenly spaced indices into n elements, the first 0 and the last n - 1.  Computed in int64: a float32
    linspace rounds n - 1 up to n above 2^24 elements (a Wan-1.3B-81f hidden state has 50_319_360), one past the end."""
    k = min(k, n)
    return torch.arange(k, dtype=torch.int64, device=device) * (n - 1) // max(k - 1, 1)


def check_rank_coherence(x: torch.Tensor) -> None:
    """Every sequence-parallel rank must enter the transformer with the SAME hidden states (the ranks keep whole latents and
    cut tokens inside the model): compare a fixed strided SAMPLE of `COHERENCE_SAMPLE` elements across ranks, element by element,
    to 1 % of the sample's largest magnitude.  A checksum would not do: the signed sum and the abs-sum of two
    differently seeded noise tensors differ by ~sqrt(N) against N -- 1e-4 relative at the 5e7..4e8 elements of a Wan / Hunyuan
    hidden state, under any tolerance that lets identical latents through a conv / GEMM whose kernel choice differs between
    processes -- while single elements of identical latents agree to an ulp (<= 0.8 % in bf16) and those of different noise
    differ by their own magnitude, whatever N.  Raises RuntimeError naming the cause (non-finite values are told apart)."""
    flat = x.reshape(-1)
    n = flat.numel()
    idx = coherence_sample_indices(n, device=x.device)
    sample = flat[idx].float()
    finite = torch.isfinite(x.float().abs().max()).float().reshape(1)
    from ..ulysses import all_gather
    every = all_gather(torch.cat([sample, finite]).reshape(1, -1), dim=0).cpu()  # (P, sample + 1): the one read-back
    if not bool((every[:, -1] > 0).all()) or not bool(torch.isfinite(every).all()):
        raise RuntimeError(
            f"the hidden states entering the transformer are not finite on some rank (finite flags {every[:, -1].tolist()}): "
            "NaN / inf in the latents or the patch embedding, not a rank-coherence problem")
    vals = every[:, :-1]
    tol = 1e-2 * vals.abs().max() + 1e-6
    worst = (vals - vals[:1]).abs().max(dim=1).values
    if not bool((worst <= tol).all()):
        raise RuntimeError(
            "sequence-parallel ranks entered the transformer with different latents (largest difference from rank 0 over "
            f"{vals.shape[1]} sampled elements, per rank: {worst.tolist()}, tolerance {float(tol):.3g}): pass the pipeline a "
            "generator seeded identically on every rank, or none")


def install_token_shard(model: nn.Module, first_block: nn.Module, gather_before: Optional[nn.Module] = None,
                        gather_after: Optional[nn.Module] = None) -> None:
    """Token-level sequence-parallel shard INSIDE the transformer (replaces the frame shard of
    pipeline_hunyuan.py:367-369 for pipeline calls).  The reference shards the latent FRAMES, which refuses every frame
    count P does not divide (129 frames -> 33 latent frames: P = 2, 4, 8 all fail) -- while the token count divides
    (S = 118 800 = 8 x 14 850).  In token mode (`ctx.sp_token_shard`, set by the pipeline call) every rank keeps the
    whole latent; the stock forward embeds it, builds the global rotary table and the global attention mask as in the
    single-process case; the token sequence is cut to this rank's contiguous chunk [r S/P, (r+1) S/P) at the first
    block's input and concatenated again (all-gather along tokens) in front of `gather_before` (the output norm).  The
    blocks in between see exactly what they see under a frame shard: a contiguous S/P chunk + the replicated text.
    `gather_after` instead of `gather_before`: concatenate the OUTPUT of that module (Wan: the last block, whose 16-bit
    output the stock forward widens to fp32 in front of the output norm -- gathering there moves half the bytes).
    Every rank must enter with the same tokens: the first cut of a pipeline call compares a checksum of the sequence
    over the group and refuses to continue on a mismatch (a generator seeded per rank would otherwise make every rank
    denoise a different video outside its own chunk).
    A training loop asks for the same mode with `token_sharded(model)`; cut and gather carry autograd as they stand (a
    slice; `ulysses.all_gather`, whose backward is the rank's own slice), and that docstring says what a rank's gradients
    then are.  The mode is the FORWARD's (`StepContext.token_shard_of`), not the flag's at the moment a hook runs."""
    from ..ulysses import all_gather
    ctx = context_of(model)
    if (gather_before is None) == (gather_after is None):
        raise ValueError("install_token_shard takes exactly one of gather_before / gather_after")

    def _swap(args, kwargs, fn):
        if "hidden_states" in kwargs:
            kwargs = dict(kwargs, hidden_states=fn(kwargs["hidden_states"]))
            return args, kwargs
        return (fn(args[0]),) + tuple(args[1:]), kwargs

    def cut(module, args, kwargs):
        if not (SP_STATE.enabled and ctx.token_shard_of(args, kwargs)):
            return None
        P, r = SP_STATE.sp_size, SP_STATE.group_local_rank

        def f(x):
            S = x.shape[1]
            if S % P:
                raise ValueError(f"{S} video tokens do not divide over {P} sequence-parallel ranks")
            if not ctx.sp_coherent:  # once per pipeline call / `token_sharded` entry: one read-back of 65 P floats
                with torch.no_grad():  # (the comparison gathers through `ulysses.all_gather`, an autograd function)
                    check_rank_coherence(x)
                ctx.sp_coherent = True
            n = S // P
            return x[:, r * n:(r + 1) * n]
        return _swap(args, kwargs, f)

    def join(module, args, kwargs):
        if not (SP_STATE.enabled and ctx.token_shard_of(args, kwargs)):
            return None
        return _swap(args, kwargs, lambda x: all_gather(x.contiguous(), dim=1))

    def join_out(module, args, output):
        if not (SP_STATE.enabled and ctx.token_shard_of(args)):
            return None
        if isinstance(output, tuple):
            return (all_gather(output[0].contiguous(), dim=1),) + tuple(output[1:])
        return all_gather(output.contiguous(), dim=1)

    add_hook(model, first_block.register_forward_pre_hook(cut, with_kwargs=True))
    if gather_before is not None:
        add_hook(model, gather_before.register_forward_pre_hook(join, with_kwargs=True))
    else:
        add_hook(model, gather_after.register_forward_hook(join_out))
