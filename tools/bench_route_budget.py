# What does routing (precision, expert) pairs by a COST BUDGET cost beside routing them by the error bound?
# (routed.route_by_fidelity(max_cost_share=...), vorta_route_budget_tiers)
#
# One layer of a headline shape, white-noise inputs, in one process with the arms alternating over --rounds rounds (device
# events around every call; median, min, max): measure-and-route by `max_cost_share` against measure-and-route by
# `max_rel_error`, both over the tiers of the configuration's precision and on the same n = 512 sampled rows (hunyuan-129f:
# fp16, 24 heads, "i8pv" -> tiers i8pv, native; wan14b-81f: bf16, 40 heads, "auto8" -> i8pv, fp8pv, native); and
# `ops.route_budget_tiers` alone beside `ops.route_fidelity_tiers` alone on records that are already there, the kernels' own
# launch-to-finish times.  The criterion is the README's for routing kernels: the difference of the two measure-and-route
# medians lies inside the min-max spread of the bound arm.
#
# usage: python tools/bench_route_budget.py --config hunyuan-129f --config wan14b-81f --out profiles/route_budget_timing.json
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402  (the headline configurations)
from bench_measured_precision import PRECISION_OF, _layer  # noqa: E402  (one layer of a configuration)
from bench_routed_fidelity import _alternate  # noqa: E402  (arms in turn, device events, medians)

N_ROWS = 512


def cost_of(a, config):
    from vorta_amd import ops
    from vorta_amd.patch.fidelity import expert_work
    from vorta_amd.routed import TIERS_OF_PRECISION, route_by_fidelity, sample_rows
    cfg, dev, dt, S, H, q, k, v, geom, kw = _layer(config)
    tiers = TIERS_OF_PRECISION[PRECISION_OF.get(config, "i8pv")]
    work = expert_work(geom, kw["text_valid"])
    rows = sample_rows(S, N_ROWS, 0, dev)
    geom.sample_tables(kw["text_valid"], rows)  # (host work, once per table: not part of a call)
    routes = route_by_fidelity(q, k, v, geom, rows=rows, max_cost_share=a.share, tiers=tiers, **kw)
    arms = {
        "by_max_rel_error": lambda: route_by_fidelity(q, k, v, geom, rows=rows, max_rel_error=a.bound, tiers=tiers, **kw),
        "by_max_cost_share": lambda: route_by_fidelity(q, k, v, geom, rows=rows, max_cost_share=a.share, tiers=tiers, **kw),
        "route_fidelity_tiers_alone": lambda: ops.route_fidelity_tiers(routes.fids, max_rel_error=a.bound, work=work),
        "route_budget_tiers_alone": lambda: ops.route_budget_tiers(routes.fids, max_cost_share=a.share, work=work),
    }
    res = _alternate(arms, a.rounds)
    bound, budget = res["by_max_rel_error"], res["by_max_cost_share"]
    extra, spread = budget["median_ms"] - bound["median_ms"], bound["max_ms"] - bound["min_ms"]
    share = ops.route_budget_tiers(routes.fids, max_cost_share=a.share, work=work, cost_share=True)
    return {"config": config, "dtype": str(dt), "precision": PRECISION_OF.get(config, "i8pv"), "tiers": list(tiers),
            "inputs": "white noise", "S": S, "heads": H, "n_rows": N_ROWS, "max_rel_error": a.bound, "max_cost_share": a.share,
            "level": float(share[4]), "cost_share": float(share[5]), "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
            "arms": res,
            "budget_against_bound": dict(extra_ms=round(extra, 4), spread_of_bound_arm_ms=round(spread, 4),
                                         inside_the_spread=bool(abs(extra) <= spread)),
            "route_kernels_alone_ms": dict(route_fidelity_tiers=res["route_fidelity_tiers_alone"],
                                           route_budget_tiers=res["route_budget_tiers_alone"]),
            "note": "device events around every call; the two measure-and-route arms differ in the routing kernel alone: "
                    "vorta_route_budget_tiers (one workgroup, 32 + 1 + 11 passes over LDS) in the place of "
                    "vorta_route_fidelity_tiers (one pass), and one more float32 allocation (the level)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(bench.CONFIGS), help="repeatable; default: hunyuan-129f")
    ap.add_argument("--bound", type=float, default=0.05)
    ap.add_argument("--share", type=float, default=0.4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_route_budget.py measures on the GPU: there is no CPU path")
    doc = {"tool": "tools/bench_route_budget.py", "runs": [cost_of(a, c) for c in (a.config or ["hunyuan-129f"])]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
