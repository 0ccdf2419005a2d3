# What does measuring the routed output cost, and what is a sample of rows worth?  (routed.routed_attention(fidelity=...),
# vorta_sampled_fidelity)
#
#   cost      one layer of a headline shape (hunyuan-129f: fp16, 8/8/8 heads, text 256 / 96, native precision; wan14b-81f: bf16,
#             14/13/13 heads, precision i8pv): the routed call WITH a sink against the SAME call without one, in one process, the
#             arms alternating over --rounds rounds (device events around every call; the median over the rounds is reported),
#             for n in {512, 2048, 8192} sampled rows and the heads "sparse" / "all".  The reference launches have one placement
#             in this build (launches of their own after the routed grid); the two arms per (n, heads) are their keys cut
#             into routed.FIDELITY_REF_SPLITS parts (the default: 8) and left whole (1).  The head lists are the route plan's
#             form, device lists with device counts (--lists device: what vorta.patch.routed_fidelity runs), or host counts
#             (--lists host).  Then the compare kernel alone, as bytes per second, beside vorta_expert_fidelity's rate on
#             full-size buffers on the same box.  Several --config: one report each, in the "runs" of one file.
#   accuracy  wan1.3b-49f (S = 8 320: every row is affordable), the generators of tests/_structured_inputs.py at 10 % noise, a
#             uniform 4/4/4 mix with every head on the expert whose assumption it meets: per head the sampled rel_error for n
#             in {256, 1024, 2048} and five seeds beside the all-rows value (n = S); the worst and the median ratio are stated.
#
# usage: python tools/bench_routed_fidelity.py cost --config hunyuan-129f --config wan14b-81f --out profiles/routed_fidelity_timing.json
#        python tools/bench_routed_fidelity.py accuracy --out profiles/routed_fidelity_accuracy.txt
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402  (the headline configurations and the mixes)

PRECISION = {"hunyuan-129f": "native", "wan14b-81f": "i8pv"}
SAMPLES = (512, 2048, 8192)


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def _alternate(arms, rounds):
    """{name: median ms} of the callables `arms`, run in turn `rounds` times after one warm-up pass of every arm"""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    events = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            events[name].append(_event_ms(fn))
    torch.cuda.synchronize()
    ms = {name: [a.elapsed_time(b) for a, b in ev] for name, ev in events.items()}
    return {name: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for name, v in ms.items()}


def cost(a):
    configs = a.config or ["hunyuan-129f"]
    doc = {"tool": "tools/bench_routed_fidelity.py cost", "runs": [cost_of(a, config) for config in configs]}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def cost_of(a, config):
    from vorta_amd import _C, ops, routed
    from vorta_amd.routed import HeadRouting, geometry_for, routed_attention, sample_rows
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
    if a.lists == "device":  # the route plan's form: (3, H) lists and a device count per expert, no host count
        routing = HeadRouting.from_device(routing.lists, torch.tensor(routing.counts_host, dtype=torch.int32, device=dev))
    precision = a.precision or PRECISION.get(config, "native")
    kw = dict(model=cfg["model"], text_len=T, text_valid=te, out=out, fp8=precision)
    def with_sink(rows, heads, splits):
        routed.FIDELITY_REF_SPLITS = splits  # the reference launches' keys: cut into 8 parts (the default), or whole (1)
        routed_attention(q, k, v, routing, geom, fidelity=[], fidelity_rows=rows, fidelity_heads=heads, **kw)

    default_splits = routed.FIDELITY_REF_SPLITS
    arms = {"plain": lambda: routed_attention(q, k, v, routing, geom, **kw)}
    for n in SAMPLES:
        rows = sample_rows(S, n, 0, dev)
        for heads in ("sparse", "all"):
            arms[f"n{n}_{heads}"] = lambda rows=rows, heads=heads: with_sink(rows, heads, default_splits)
            arms[f"n{n}_{heads}_whole_keys"] = lambda rows=rows, heads=heads: with_sink(rows, heads, 1)
    res = _alternate(arms, a.rounds)
    plain = res["plain"]["median_ms"]
    counts = [experts.count(e) for e in range(3)]
    per_head_dense = 4.0 * (S + te) ** 2 * 128
    routed_flops = bench.algorithmic_flops(cfg, np.asarray(experts))[0]  # the work formulas of BASELINE.md section 2
    routed.FIDELITY_REF_SPLITS = default_splits
    report = {"config": config, "dtype": str(dt), "precision": precision, "heads": counts, "S": S, "text": [T, te],
              "head_lists": a.lists, "reference_key_parts": routed.fidelity_ref_splits(S + te),
              "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "placement": "after the routed grid (the only one built)",
              "arms": res, "overhead": {}}
    for n in SAMPLES:
        for heads in ("sparse", "all"):
            m = res[f"n{n}_{heads}"]["median_ms"]
            measured = H - counts[0] if heads == "sparse" else H
            whole = res[f"n{n}_{heads}_whole_keys"]["median_ms"]
            report["overhead"][f"n{n}_{heads}"] = dict(
                extra_ms=round(m - plain, 4), ratio_to_plain=round(m / plain, 4), measured_heads=measured,
                whole_keys_extra_ms=round(whole - plain, 4), whole_keys_ratio_to_plain=round(whole / plain, 4),
                flop_expectation_of_a_dense_layer=round(measured * n / (H * float(S + te)), 5))
    report["plain_tflops"] = round(routed_flops / (plain * 1e-3) / 1e12, 1)
    report["dense_head_flops"] = per_head_dense
    # the compare kernel alone, and vorta_expert_fidelity on full-size buffers of 8 heads (four tensors read once each)
    Hc = 8
    bufs = [torch.randn((Hc, S + T, 128), generator=gen, device=dev, dtype=dt) for _ in range(4)]
    cmp_arms = {"expert_fidelity_full_size": lambda: ops.expert_fidelity(bufs[:3], bufs[3])}
    for n in SAMPLES:
        rows = sample_rows(S, n, 0, dev)
        ref = torch.randn((H, n, 128), generator=gen, device=dev, dtype=dt)
        cmp_arms[f"sampled_fidelity_n{n}"] = lambda ref=ref, rows=rows: ops.sampled_fidelity(ref, out[0], rows)
    cres = _alternate(cmp_arms, max(a.rounds, 5))
    ef = cres["expert_fidelity_full_size"]["median_ms"]
    report["compare_kernel"] = {"expert_fidelity_full_size": dict(cres["expert_fidelity_full_size"], bytes=4 * Hc * (S + T) * 256,
                                                                  gb_per_s=round(4 * Hc * (S + T) * 256 / (ef * 1e-3) / 1e9, 1))}
    for n in SAMPLES:
        m = cres[f"sampled_fidelity_n{n}"]["median_ms"]
        nbytes = 2 * H * n * 256
        report["compare_kernel"][f"sampled_fidelity_n{n}"] = dict(cres[f"sampled_fidelity_n{n}"], bytes=nbytes, heads=H,
                                                                 partials=H * _C.SAMPLED_FIDELITY_PARTS,
                                                                 gb_per_s=round(nbytes / (m * 1e-3) / 1e9, 1))
    report["note"] = ("device events around every call, launch overhead and the two small allocations of a sink included; the "
                      "compare figures are whole calls (partial launch + join + the NaN fills), not kernel times")
    return report


def accuracy(a):
    import _structured_inputs as SI
    from vorta_amd.routed import HeadRouting, geometry_for, routed_attention, sample_rows
    cfg = bench.CONFIGS["wan1.3b-49f"]
    dev = torch.device("cuda:0")
    latent, tile, group = cfg["latent"], cfg["tile"], cfg["group"]
    S, H = latent[0] * latent[1] * latent[2], cfg["heads"]
    experts = [0, 1, 2] * (H // 3)
    gen = torch.Generator(device=dev).manual_seed(1234)
    q, k, v = (x.to(torch.bfloat16) for x in SI.structured_layer(latent, experts, tile, group, a.noise, gen, dev))
    geom = geometry_for(latent, tile, cfg["window"], group, cfg["rate"], dev)
    routing = HeadRouting.from_expert_ids(experts, dev)
    lines = [f"tools/bench_routed_fidelity.py accuracy: wan1.3b-49f latent {latent} (S = {S}), tile {tile}, coreset window {group}, "
             f"{H} heads {experts}, bf16,",
             f"structured inputs (tests/_structured_inputs.py, every head on the expert whose assumption it meets) at noise {a.noise}, "
             f"{torch.cuda.get_device_name(0)}"]
    for precision in ("native", "i8pv"):
        def rel(n, seed):
            sink = []
            routed_attention(q, k, v, routing, geom, model="wan", fp8=precision, fidelity=sink,
                             fidelity_rows=sample_rows(S, n, seed, dev), fidelity_heads="all")
            return sink[0].rel_error().double().cpu().numpy()

        full = rel(S, 0)
        lines.append(f"\nprecision {precision}: rel_error over ALL rows (n = S) per head")
        lines.append("  " + " ".join(f"{x:.5f}" for x in full))
        ok = full > 0  # (a native full-attention head reproduces the dense rows bit for bit: 0 / 0 is no ratio)
        for n in (256, 1024, 2048):
            ratios = []
            for seed in range(5):
                r = rel(n, seed)
                ratios.append(r[ok] / full[ok])
                lines.append(f"  n {n:5d} seed {seed}: " + " ".join(f"{x:.5f}" for x in r))
            ratios = np.concatenate(ratios)
            worst = ratios[np.argmax(np.abs(ratios - 1.0))]  # the ratio farthest from 1
            lines.append(f"  n {n:5d}: sampled / all-rows rel_error over {ratios.size} (head, seed) pairs with a non-zero all-rows "
                         f"error: median {np.median(ratios):.4f}, min {ratios.min():.4f}, max {ratios.max():.4f}, worst {worst:.4f}")
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
    c.add_argument("--lists", default="device", choices=("device", "host"), help="head lists with device counts (the patch "
                   "layer's route plan) or with host counts")
    c.add_argument("--precision", default="", help="default: native for hunyuan-129f, i8pv for wan14b-81f")
    c.add_argument("--rounds", type=int, default=5)
    c.add_argument("--out", default="")
    c.set_defaults(fn=cost)
    acc = sub.add_parser("accuracy")
    acc.add_argument("--noise", type=float, default=0.10)
    acc.add_argument("--out", default="")
    acc.set_defaults(fn=accuracy)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_routed_fidelity.py measures on the GPU: there is no CPU path")
    a.fn(a)


if __name__ == "__main__":
    main()
