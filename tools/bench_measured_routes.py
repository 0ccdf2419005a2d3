# What does routing a layer by its own measurement cost, and what does the bound hold on ALL rows?  (routed.route_by_fidelity,
# vorta_route_fidelity)
#
#   cost      one layer of a headline shape (hunyuan-129f: fp16, text 256 / 96; wan14b-81f: bf16), native precision, white-noise
#             inputs, in one process with the arms alternating over --rounds rounds (device events around every call; median, min, max):
#             (a) `routed.sampled_expert_fidelity(out=None)` alone against `routed.route_by_fidelity` alone, n in {512, 2048}:
#                 the difference is the new kernel (+ its three output allocations); and `ops.route_fidelity` alone on a record
#                 that is already there, the kernel's own launch-to-finish time;
#             (b) one routed layer under `max_flops_share` = the share of the configuration's uniform split (measure at n = 512,
#                 route, launch) against the same layer launched by device head lists of that split.
#   accuracy  wan1.3b-49f (S = 8 320), the generators of tests/_structured_inputs.py at 10 / 3 / 1 % noise, bounds 0.02 / 0.05 / 0.1 at
#             n = 512: the table, its flops_share, and per sparse head the all-rows rel_error of the routed output
#             (routed_attention(fidelity=..., fidelity_rows=S)) beside the sampled one the route was chosen by.
#
# usage: python tools/bench_measured_routes.py cost --config hunyuan-129f --config wan14b-81f --out profiles/measured_routes_timing.json
#        python tools/bench_measured_routes.py accuracy --out profiles/measured_routes_accuracy.txt
import argparse
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402  (the headline configurations and the mixes)
from bench_routed_fidelity import _alternate  # noqa: E402  (arms in turn, device events, medians)

SAMPLES = (512, 2048)


def cost_of(a, config):
    from vorta_amd import ops
    from vorta_amd.patch.fidelity import expert_work
    from vorta_amd.routed import (HeadRouting, geometry_for, route_by_fidelity, routed_attention, sample_rows,
                                  sampled_expert_fidelity)
    cfg = bench.CONFIGS[config]
    dev = torch.device("cuda:0")
    dt = torch.float16 if cfg["dtype"] == "fp16" else torch.bfloat16
    S = cfg["latent"][0] * cfg["latent"][1] * cfg["latent"][2]
    T, te, H = cfg["text"], cfg["text_valid"], cfg["heads"]
    experts = [int(e) for e in bench.layer_experts(cfg, "uniform", 0)]
    gen = torch.Generator(device=dev).manual_seed(7)
    q, k, v = (torch.randn((1, H, S + T, 128), generator=gen, device=dev, dtype=dt) for _ in range(3))
    out = torch.empty_like(q)
    geom = geometry_for(cfg["latent"], cfg["tile"], cfg["window"], cfg["group"], cfg["rate"], dev)
    geom.prebuild(te)
    routing = HeadRouting.from_expert_ids(experts, dev)
    routing = HeadRouting.from_device(routing.lists, torch.tensor(routing.counts_host, dtype=torch.int32, device=dev))
    kw = dict(model=cfg["model"], text_len=T, text_valid=te)
    work = expert_work(geom, te)
    share = sum(work[e] for e in experts) / (H * work[0])
    rows = {n: sample_rows(S, n, 0, dev) for n in SAMPLES}
    for r in rows.values():
        geom.sample_tables(te, r)  # (host work, once per table: not part of a call)
    arms = {}
    for n in SAMPLES:
        arms[f"sampled_expert_fidelity_n{n}"] = lambda r=rows[n]: sampled_expert_fidelity(q, k, v, geom, rows=r, **kw)
        arms[f"route_by_fidelity_n{n}"] = lambda r=rows[n]: route_by_fidelity(q, k, v, geom, rows=r, max_rel_error=0.05, **kw)
    record = sampled_expert_fidelity(q, k, v, geom, rows=rows[SAMPLES[0]], **kw)
    arms["route_fidelity_alone"] = lambda: ops.route_fidelity(record, max_rel_error=0.05, work=work)  # the kernel + its allocations
    arms["layer_by_device_lists"] = lambda: routed_attention(q, k, v, routing, geom, out=out, fp8="native", **kw)

    def layer_by_budget():
        measured = route_by_fidelity(q, k, v, geom, rows=rows[SAMPLES[0]], max_flops_share=share, **kw)[0]
        routed_attention(q, k, v, measured, geom, out=out, fp8="native", **kw)

    arms["layer_by_flops_share"] = layer_by_budget
    res = _alternate(arms, a.rounds)
    counts = route_by_fidelity(q, k, v, geom, rows=rows[SAMPLES[0]], max_flops_share=share, **kw)[0].counts_dev.tolist()
    report = {"config": config, "dtype": str(dt), "precision": "native", "inputs": "white noise", "S": S, "text": [T, te],
              "uniform_split": [experts.count(e) for e in range(3)], "max_flops_share": round(share, 6),
              "heads_under_that_share": counts, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "arms": res,
              "route_kernel": {}}
    for n in SAMPLES:
        sef, rbf = res[f"sampled_expert_fidelity_n{n}"], res[f"route_by_fidelity_n{n}"]
        extra = rbf["median_ms"] - sef["median_ms"]
        report["route_kernel"][f"n{n}"] = dict(
            extra_ms=round(extra, 4), spread_of_sampled_expert_fidelity_ms=round(sef["max_ms"] - sef["min_ms"], 4),
            inside_the_spread=bool(abs(extra) <= sef["max_ms"] - sef["min_ms"]))
    report["route_kernel"]["alone_ms"] = res["route_fidelity_alone"]
    lists, budget = res["layer_by_device_lists"]["median_ms"], res["layer_by_flops_share"]["median_ms"]
    report["layer"] = dict(extra_ms=round(budget - lists, 4), ratio=round(budget / lists, 4))
    report["note"] = ("device events around every call; route_by_fidelity = sampled_expert_fidelity + vorta_route_fidelity (one "
                      "workgroup) + three small allocations; the layer under a share launches the heads the rule moved, which on "
                      "white noise need not be the uniform split's heads or experts")
    return report


def cost(a):
    doc = {"tool": "tools/bench_measured_routes.py cost", "runs": [cost_of(a, c) for c in (a.config or ["hunyuan-129f"])]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def accuracy(a):
    import _structured_inputs as SI
    from vorta_amd import ops
    from vorta_amd.patch.fidelity import expert_work
    from vorta_amd.routed import geometry_for, route_by_fidelity, routed_attention, sample_rows
    cfg = bench.CONFIGS["wan1.3b-49f"]
    dev = torch.device("cuda:0")
    latent, tile, group = cfg["latent"], cfg["tile"], cfg["group"]
    S, H = latent[0] * latent[1] * latent[2], cfg["heads"]
    built_for = [0, 1, 2] * (H // 3)
    geom = geometry_for(latent, tile, cfg["window"], group, cfg["rate"], dev)
    work = expert_work(geom, 0)
    rows = sample_rows(S, a.rows, 0, dev)
    lines = [f"tools/bench_measured_routes.py accuracy: wan1.3b-49f latent {latent} (S = {S}), tile {tile}, coreset window {group}, "
             f"{H} heads, bf16,",
             f"structured inputs (tests/_structured_inputs.py, head h built for expert {built_for}), "
             f"n = {a.rows} sampled rows (seed 0), {torch.cuda.get_device_name(0)}",
             f"work of one head under expert 0 / 1 / 2 relative to full attention: {[round(w / work[0], 4) for w in work]}"]
    for noise in a.noise or [0.10, 0.03, 0.01]:
        gen = torch.Generator(device=dev).manual_seed(1234)
        q, k, v = (x.to(torch.bfloat16) for x in SI.structured_layer(latent, built_for, tile, group, noise, gen, dev))
        for bound in a.bound or [0.02, 0.05, 0.1]:
            routing, ids, fid = route_by_fidelity(q, k, v, geom, model="wan", rows=rows, max_rel_error=bound)
            share = float(ops.route_fidelity(fid, max_rel_error=bound, work=work, flops_share=True)[3])
            sink = []
            routed_attention(q, k, v, routing, geom, model="wan", fp8="native", fidelity=sink, fidelity_rows=sample_rows(S, S, 0, dev))
            table, sampled, every = ids.tolist(), fid.rel_error().cpu(), sink[0].rel_error().cpu()
            if bound == (a.bound or [0.02])[0]:  # the record does not depend on the bound: once per noise level
                lines += [f"\n==== noise {noise}: sampled rel_error per head, coreset | sliding tile",
                          "  " + " ".join(f"{x:.5f}" for x in sampled[:, 0].tolist()),
                          "  " + " ".join(f"{x:.5f}" for x in sampled[:, 1].tolist())]
            lines += [f"\nnoise {noise}, max_rel_error {bound}: table {table}", f"  flops_share {share:.6f}",
                      "  sparse head: expert, rel_error on the sampled rows (what the route was chosen by) | rel_error of the "
                      "routed output on ALL rows"]
            worst = 0.0
            for h, e in enumerate(table):
                if e:
                    lines.append(f"    head {h:2d}: expert {e}, {float(sampled[h, e - 1]):.5f} | {float(every[h]):.5f}")
                    worst = max(worst, float(every[h]))
            lines.append(f"  worst all-rows rel_error of a sparse head: {worst:.5f} (bound {bound})" if any(table) else
                         "  no sparse head")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="what", required=True)
    c = sub.add_parser("cost")
    c.add_argument("--config", action="append", choices=sorted(bench.CONFIGS), help="repeatable; default: hunyuan-129f")
    c.add_argument("--rounds", type=int, default=7)
    c.add_argument("--out", default="")
    c.set_defaults(fn=cost)
    acc = sub.add_parser("accuracy")
    acc.add_argument("--noise", type=float, action="append", help="repeatable; default: 0.10, 0.03, 0.01")
    acc.add_argument("--bound", type=float, action="append", help="repeatable; default: 0.02, 0.05, 0.1")
    acc.add_argument("--rows", type=int, default=512)
    acc.add_argument("--out", default="")
    acc.set_defaults(fn=accuracy)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_measured_routes.py measures on the GPU: there is no CPU path")
    a.fn(a)


if __name__ == "__main__":
    main()
