# What does routing every head's PRECISION by the measured bound cost, and what do the launches then hold?
# (routed.route_by_fidelity(tiers=...), vorta_route_fidelity_tiers, routed.routed_attention_tiers)
#
#   cost      one layer of a headline shape, white-noise inputs, in one process with the arms alternating over --rounds rounds
#             (device events around every call; median, min, max): measure-and-route over the tiers of the configuration's
#             precision against measure-and-route over experts alone (the parent's `route_by_fidelity`), n in {512, 2048}
#             (hunyuan-129f: fp16, 24 heads, "i8pv" -> tiers i8pv, native; wan14b-81f: bf16, 40 heads, "auto8" -> i8pv, fp8pv,
#             native); and `ops.route_fidelity_tiers` alone beside `ops.route_fidelity` alone on records that are already there,
#             the kernels' own launch-to-finish times.
#   accuracy  the same shapes and inputs: the (expert, tier) table under --bound, and per head the rel_error of what was
#             LAUNCHED (routed_attention_tiers(fidelity=..., fidelity_heads="all") on the same rows) beside the candidate's
#             the route was chosen by, and their ratio.
#
# usage: python tools/bench_measured_precision.py cost --config hunyuan-129f --config wan14b-81f --out profiles/measured_precision_timing.json
#        python tools/bench_measured_precision.py accuracy --config hunyuan-129f --config wan14b-81f --out profiles/measured_precision_accuracy.txt
import argparse
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402  (the headline configurations)
from bench_routed_fidelity import _alternate  # noqa: E402  (arms in turn, device events, medians)

SAMPLES = (512, 2048)
PRECISION_OF = {"hunyuan-129f": "i8pv", "wan14b-81f": "auto8"}


def _layer(config):
    from vorta_amd.routed import geometry_for
    cfg = bench.CONFIGS[config]
    dev = torch.device("cuda:0")
    dt = torch.float16 if cfg["dtype"] == "fp16" else torch.bfloat16
    S = cfg["latent"][0] * cfg["latent"][1] * cfg["latent"][2]
    T, te, H = cfg["text"], cfg["text_valid"], cfg["heads"]
    gen = torch.Generator(device=dev).manual_seed(7)
    q, k, v = (torch.randn((1, H, S + T, 128), generator=gen, device=dev, dtype=dt) for _ in range(3))
    geom = geometry_for(cfg["latent"], cfg["tile"], cfg["window"], cfg["group"], cfg["rate"], dev)
    geom.prebuild(te)
    return cfg, dev, dt, S, H, q, k, v, geom, dict(model=cfg["model"], text_len=T, text_valid=te)


def cost_of(a, config):
    from vorta_amd import ops
    from vorta_amd.patch.fidelity import expert_work
    from vorta_amd.routed import TIERS_OF_PRECISION, route_by_fidelity, sample_rows
    cfg, dev, dt, S, H, q, k, v, geom, kw = _layer(config)
    tiers = TIERS_OF_PRECISION[PRECISION_OF.get(config, "i8pv")]
    work = expert_work(geom, kw["text_valid"])
    rows = {n: sample_rows(S, n, 0, dev) for n in SAMPLES}
    for r in rows.values():
        geom.sample_tables(kw["text_valid"], r)  # (host work, once per table: not part of a call)
    arms = {}
    for n in SAMPLES:
        arms[f"route_by_fidelity_n{n}"] = lambda r=rows[n]: route_by_fidelity(q, k, v, geom, rows=r, max_rel_error=a.bound, **kw)
        arms[f"route_by_fidelity_tiers_n{n}"] = lambda r=rows[n]: route_by_fidelity(q, k, v, geom, rows=r, max_rel_error=a.bound,
                                                                                    tiers=tiers, **kw)
    routes = route_by_fidelity(q, k, v, geom, rows=rows[SAMPLES[0]], max_rel_error=a.bound, tiers=tiers, **kw)
    arms["route_fidelity_alone"] = lambda: ops.route_fidelity(routes.fids["native"], max_rel_error=a.bound, work=work)
    arms["route_fidelity_tiers_alone"] = lambda: ops.route_fidelity_tiers(routes.fids, max_rel_error=a.bound, work=work)
    res = _alternate(arms, a.rounds)
    report = {"config": config, "dtype": str(dt), "precision": PRECISION_OF.get(config, "i8pv"), "tiers": list(tiers),
              "inputs": "white noise", "S": S, "heads": H, "max_rel_error": a.bound, "rounds": a.rounds,
              "device": torch.cuda.get_device_name(0), "arms": res, "tiers_against_experts_alone": {}}
    for n in SAMPLES:
        base, tier = res[f"route_by_fidelity_n{n}"], res[f"route_by_fidelity_tiers_n{n}"]
        report["tiers_against_experts_alone"][f"n{n}"] = dict(
            extra_ms=round(tier["median_ms"] - base["median_ms"], 4), ratio=round(tier["median_ms"] / base["median_ms"], 4),
            spread_of_experts_alone_ms=round(base["max_ms"] - base["min_ms"], 4),
            spread_of_tiers_ms=round(tier["max_ms"] - tier["min_ms"], 4))
    report["route_kernels_alone_ms"] = dict(route_fidelity=res["route_fidelity_alone"], route_fidelity_tiers=res["route_fidelity_tiers_alone"])
    report["note"] = ("device events around every call; measure-and-route over tiers = the native measurement + one measurement per "
                      "8-bit tier (K, V converted once per call) + vorta_route_fidelity_tiers (one workgroup) + a stack of the "
                      "records and four small allocations")
    return report


def cost(a):
    doc = {"tool": "tools/bench_measured_precision.py cost", "runs": [cost_of(a, c) for c in (a.config or ["hunyuan-129f"])]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def accuracy_of(a, config, lines):
    from vorta_amd import ops
    from vorta_amd.routed import TIERS_OF_PRECISION, route_by_fidelity, routed_attention_tiers, sample_rows
    cfg, dev, dt, S, H, q, k, v, geom, kw = _layer(config)
    tiers = TIERS_OF_PRECISION[PRECISION_OF.get(config, "i8pv")]
    lines += [f"\n==== {config}: latent {cfg['latent']} (S = {S}), {H} heads, {dt}, white noise, tiers {tiers}, "
              f"max_rel_error {a.bound}, {torch.cuda.get_device_name(0)}"]
    for n in SAMPLES:
        rows = sample_rows(S, n, 0, dev)
        routes = route_by_fidelity(q, k, v, geom, rows=rows, max_rel_error=a.bound, tiers=tiers, **kw)
        sink = []
        routed_attention_tiers(q, k, v, routes.routings, geom, operands=routes.operands, fidelity=sink, fidelity_rows=rows,
                               fidelity_heads="all", **kw)
        experts, tier_ids, launched = routes.expert_ids.tolist(), routes.tier_ids.tolist(), sink[0].rel_error().cpu().tolist()
        rel = {t: f.rel_error().cpu() for t, f in routes.fids.items()}
        lines += [f"\nn = {n} sampled rows (seed 0)", f"  experts {experts}", f"  tiers   {tier_ids}  (0 native, 1 fp8pv, 2 i8pv)",
                  "  counts per tier (full, coreset, sliding): " + ", ".join(f"{t} {c}" for t, c in zip(tiers, routes.counts.tolist()))]
        for t in tiers:
            r = rel[t]
            lines.append(f"  candidates in {t}: coreset {float(r[:, 0].min()):.5f} - {float(r[:, 0].max()):.5f}, sliding "
                         f"{float(r[:, 1].min()):.5f} - {float(r[:, 1].max()):.5f}"
                         + ("" if t == "native" else f", full {float(r[:, 2].min()):.5f} - {float(r[:, 2].max()):.5f}"))
        lines.append("  head: expert, tier, candidate rel_error | launched rel_error | launched / candidate")
        ratios = []
        for h in range(H):
            name = ops.TIER_NAMES[tier_ids[h]]
            cand = 0.0 if (name == "native" and experts[h] == 0) else float(rel[name][h, 2 if experts[h] == 0 else experts[h] - 1])
            ratio = launched[h] / cand if cand > 0 else float("nan")
            ratios.append(ratio)
            lines.append(f"    head {h:2d}: expert {experts[h]}, {name:6s}, {cand:.5f} | {launched[h]:.5f} | {ratio:.4f}")
        finite = [r for r in ratios if r == r]
        over = sum(1 for x in launched if x > a.bound)
        lines.append(f"  launched / candidate: {min(finite):.4f} - {max(finite):.4f}; heads launched over the bound: {over}"
                     if finite else f"  every head on full attention in the input dtype; heads launched over the bound: {over}")


def accuracy(a):
    lines = ["tools/bench_measured_precision.py accuracy: per head the candidate the route was chosen by and what the launch wrote, "
             "both against dense attention in the input dtype on the sampled rows"]
    for config in a.config or ["hunyuan-129f"]:
        accuracy_of(a, config, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    for name, fn in (("cost", cost), ("accuracy", accuracy)):
        c = sub.add_parser(name)
        c.add_argument("--config", action="append", choices=sorted(bench.CONFIGS), help="repeatable; default: hunyuan-129f")
        c.add_argument("--bound", type=float, default=0.05)
        c.add_argument("--rounds", type=int, default=7)
        c.add_argument("--out", default="")
        c.set_defaults(fn=fn)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_measured_precision.py measures on the GPU: there is no CPU path")
    a.fn(a)


if __name__ == "__main__":
    main()
