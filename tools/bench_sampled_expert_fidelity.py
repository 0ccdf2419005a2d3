# What does the per-expert measurement on sampled rows cost, and what is the sample worth?  (routed.sampled_expert_fidelity,
# vorta_gather_sample_rows)
#
#   cost      one layer of a headline shape (hunyuan-129f: fp16, 8/8/8 heads, text 256 / 96; wan14b-81f: bf16, 14/13/13 heads), native
#             precision, in one process with the arms alternating over --rounds rounds (device events around every call; medians):
#             (a) the routed call WITH `expert_fidelity=[...]` for n in {512, 2048, 8192} against the SAME call without a sink;
#             (b) `soft_mixture_attention(fidelity=[...])`, the only other way to the same table.  Beside each n the FLOP
#             expectation: per measured head n / S of one full + one coreset + one sliding head, over the routed layer's FLOPs.
#   accuracy  wan1.3b-49f (S = 8 320), the generators of tests/_structured_inputs.py at 10 % noise: per expert the sampled
#             rel_error over the n = S value of the same function for n in {256, 1024, 2048} and five seeds, and the number of
#             heads on which routes_from_fidelity(., 0.05) differs between the sampled record and the soft mixture's.
#
# usage: python tools/bench_sampled_expert_fidelity.py cost --config hunyuan-129f --config wan14b-81f --out profiles/sampled_expert_fidelity_timing.json
#        python tools/bench_sampled_expert_fidelity.py accuracy --out profiles/sampled_expert_fidelity_accuracy.txt
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402  (the headline configurations and the mixes)
from bench_routed_fidelity import _alternate  # noqa: E402  (arms in turn, device events, medians)

SAMPLES = (512, 2048, 8192)


def cost_of(a, config):
    from vorta_amd.patch.fidelity import expert_work
    from vorta_amd.routed import HeadRouting, geometry_for, routed_attention, sample_rows, soft_mixture_attention
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
    scores = torch.full((1, H, 3), 1.0 / 3, device=dev, dtype=dt)
    arms = {"plain": lambda: routed_attention(q, k, v, routing, geom, out=out, fp8="native", **kw),
            "soft_mixture_with_fidelity": lambda: soft_mixture_attention(q, k, v, scores, geom, out=out, fidelity=[], **kw)}
    for n in SAMPLES:
        rows = sample_rows(S, n, 0, dev)
        geom.sample_tables(te, rows)  # (host work, once per table: not part of a call)
        arms[f"n{n}"] = lambda rows=rows: routed_attention(q, k, v, routing, geom, out=out, fp8="native", expert_fidelity=[],
                                                           fidelity_rows=rows, **kw)
    res = _alternate(arms, a.rounds)
    plain, soft = res["plain"]["median_ms"], res["soft_mixture_with_fidelity"]["median_ms"]
    work = expert_work(geom, te)
    routed_flops = sum(work[e] for e in experts)
    report = {"config": config, "dtype": str(dt), "precision": "native", "heads": [experts.count(e) for e in range(3)], "S": S,
              "text": [T, te], "head_lists": "device", "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "arms": res,
              "overhead": {}}
    for n in SAMPLES:
        m = res[f"n{n}"]["median_ms"]
        expected = H * (n / float(S)) * sum(work) / routed_flops  # + two selections, which are bandwidth, not FLOPs
        report["overhead"][f"n{n}"] = dict(extra_ms=round(m - plain, 4), ratio_to_plain=round(m / plain, 4),
                                           flop_expectation_ratio_to_plain=round(1 + expected, 4),
                                           measured_over_expected_extra=round((m - plain) / (expected * plain), 2),
                                           soft_mixture_over_this=round(soft / m, 2))
    report["note"] = ("device events around every call; every head of the layer is measured (all three experts + the routed rows); "
                      "the FLOP expectation prices the extra work at the plain call's own rate")
    return report


def cost(a):
    doc = {"tool": "tools/bench_sampled_expert_fidelity.py cost", "runs": [cost_of(a, c) for c in (a.config or ["hunyuan-129f"])]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def accuracy(a):
    import _structured_inputs as SI
    from vorta_amd.patch.fidelity import routes_from_fidelity
    from vorta_amd.routed import geometry_for, sample_rows, sampled_expert_fidelity, soft_mixture_attention
    cfg = bench.CONFIGS["wan1.3b-49f"]
    dev = torch.device("cuda:0")
    latent, tile, group = cfg["latent"], cfg["tile"], cfg["group"]
    S, H = latent[0] * latent[1] * latent[2], cfg["heads"]
    experts = [0, 1, 2] * (H // 3)
    gen = torch.Generator(device=dev).manual_seed(1234)
    q, k, v = (x.to(torch.bfloat16) for x in SI.structured_layer(latent, experts, tile, group, a.noise, gen, dev))
    geom = geometry_for(latent, tile, cfg["window"], group, cfg["rate"], dev)
    sink = []
    soft_mixture_attention(q, k, v, torch.full((1, H, 3), 1.0 / 3, device=dev, dtype=q.dtype), geom, model="wan", fidelity=sink)
    soft_table = routes_from_fidelity(sink[0], a.bound)
    measure = lambda n, seed: sampled_expert_fidelity(q, k, v, geom, model="wan", rows=sample_rows(S, n, seed, dev))  # noqa: E731
    full = measure(S, 0)
    full_rel = full.rel_error().double().cpu().numpy()[:, :2]
    lines = [f"tools/bench_sampled_expert_fidelity.py accuracy: wan1.3b-49f latent {latent} (S = {S}), tile {tile}, coreset window "
             f"{group}, {H} heads, bf16,",
             f"structured inputs (tests/_structured_inputs.py, head h built for expert {experts}) at noise {a.noise}, "
             f"{torch.cuda.get_device_name(0)}",
             "\nrel_error over ALL rows (n = S) per head: coreset | sliding tile",
             "  " + " ".join(f"{x:.5f}" for x in full_rel[:, 0]), "  " + " ".join(f"{x:.5f}" for x in full_rel[:, 1]),
             f"soft mixture's record, same columns (rows of the whole sequence; routes at {a.bound}: {soft_table.tolist()})",
             "  " + " ".join(f"{x:.5f}" for x in sink[0].rel_error()[:, 0].tolist()),
             "  " + " ".join(f"{x:.5f}" for x in sink[0].rel_error()[:, 1].tolist()),
             f"n = S: routes differ from the soft mixture's on {int((routes_from_fidelity(full, a.bound) != soft_table).sum())} of {H} heads"]
    for n in (256, 1024, 2048):
        ratios, differ = [[], []], []
        for seed in range(5):
            fid = measure(n, seed)
            r = fid.rel_error().double().cpu().numpy()[:, :2]
            for col in range(2):
                ratios[col].append(r[:, col] / full_rel[:, col])
            differ.append(int((routes_from_fidelity(fid, a.bound) != soft_table).sum()))
        for col, name in enumerate(("coreset", "sliding")):
            x = np.concatenate(ratios[col])
            lines.append(f"  n {n:5d} {name:8s}: sampled / all-rows rel_error over {x.size} (head, seed) pairs: median {np.median(x):.4f}, "
                         f"min {x.min():.4f}, max {x.max():.4f}")
        lines.append(f"  n {n:5d}: heads whose route at {a.bound} differs from the soft mixture's, per seed: {differ} of {H}")
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
    c.add_argument("--rounds", type=int, default=5)
    c.add_argument("--out", default="")
    c.set_defaults(fn=cost)
    acc = sub.add_parser("accuracy")
    acc.add_argument("--noise", type=float, default=0.10)
    acc.add_argument("--bound", type=float, default=0.05)
    acc.add_argument("--out", default="")
    acc.set_defaults(fn=accuracy)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampled_expert_fidelity.py measures on the GPU: there is no CPU path")
    a.fn(a)


if __name__ == "__main__":
    main()
