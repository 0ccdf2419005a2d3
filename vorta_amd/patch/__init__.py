"""vorta.patch: Router, keyword preparation, pixel->token map, and the model / pipeline entry points.

The scripts import the entry points from the submodules, as with the reference (whose `__init__` is empty):
`vorta.patch.modeling_{hunyuan,wan}.{apply_vorta_transformer, apply_sp_flashattn_transformer}`,
`vorta.patch.pipeline_{hunyuan,wan}.{vorta_pipeline_call, sp_pipeline_call, apply_vorta_pipeline}`
(scripts/hunyuan/inference.py:27-32, scripts/wan/inference.py:32-37).  They attach to the stock diffusers
forwards with hooks (vorta_amd/patch/_engine.py) and import nothing from diffusers at module level.

For router training on a patched model: `original_attention(model)` (the dense teacher pass) and `routing_scores_of(model)`
(the scores of the latest student forward, with their graph); under sequence parallelism `token_sharded(model)` (whole
latents in, tokens sharded inside the model) and `all_reduce_router_grads(model)` (the ranks' shares of the router
gradients, summed).  For judging a router or a `tau_sparse`:
`expert_fidelity(model)` / `fidelity_of(model)` (per layer and head, how far each sparse expert and the mixed output are from
full attention) and the host helpers `routes_from_fidelity` / `evaluate_routing` (patch/fidelity.py); at inference,
`routed_fidelity(model)` / `routed_fidelity_of(model)`: the routed output as run against dense attention on sampled rows;
`sampled_expert_fidelity(model)` / `sampled_expert_fidelity_of(model)`: what EVERY expert would have written on those rows (an
`ExpertFidelity` without the soft mixture's forward), and `fixed_routes(model, table)`: run the model by an expert table;
`measured_routes(model, max_rel_error=... | max_flops_share=...)` / `measured_routes_of(model)`: route every layer of every
forward by its own measurement on the device -- a stated error bound or FLOP budget, no router checkpoint, no host read;
`routes_from_fidelity_tiers`: the error-bound rule over (precision tier, expert) pairs, from one record per tier -- the
definition `ops.route_fidelity_tiers` (vorta_route_fidelity_tiers) equals on the device; `repair_routes`: which heads, as
launched, are over a stated error on the sampled rows and the routes without them -- the definition `ops.route_repair`
(vorta_route_repair) equals; `measured_routes(..., repair_above=...)` / `fixed_routes(..., repair_above=...)` verify and repair
every forward by it, and `repaired_routes_of(model)` reads the latest forward's tables;
`routes_within_cost_share`: the COST-budget rule over (precision tier, expert) pairs -- at most this share of the dense layer's
cost, any expert in any precision, the smallest largest error that buys; the definition `ops.route_budget_tiers`
(vorta_route_budget_tiers) equals -- `measured_routes(model, max_cost_share=...)` routes every layer by it and
`measured_levels_of(model)` reads the error each layer's budget bought."""
from ._engine import all_reduce_router_grads, original_attention, routing_scores_of, token_sharded
from .fidelity import (evaluate_routing, expert_fidelity, expert_work, fidelity_of, fixed_routes, measured_levels_of,
                       measured_precisions_of, measured_routes, measured_routes_of, repair_routes, repaired_routes_of,
                       routed_fidelity, routed_fidelity_of, routes_from_fidelity, routes_from_fidelity_tiers,
                       routes_within_cost_share, sampled_expert_fidelity, sampled_expert_fidelity_of)
from .router import Router, load_router_checkpoint
from .utils import (Pixel2TokenFactory, hunyuan_pixel2token, prepare_hunyuan_self_attn_kwargs,
                    prepare_wan_self_attn_kwargs, wan_pixel2token)
