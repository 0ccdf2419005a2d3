# What does verifying the launched routes on sampled rows and repairing the heads over a bound cost, and what do the launches
# hold afterwards?  (routed.routed_attention_repaired, vorta_route_repair)
#
# One layer of a headline shape, white-noise inputs, in one process with the arms alternating over --rounds rounds (device
# events around every call; median, min, max).  Per configuration and sample size n in {512, 2048}:
#   stored_today          (a) a stored-route forward as the parent launches it: the routed call over device lists, nothing more
#   repaired_none         (b) the same with repair_above and ZERO violators: the verification on the sampled rows, vorta_route_repair
#                             and the empty repair launch
#   measure_and_launch    (c) the parent's measured_routes(refresh_every=1) forward: route_by_fidelity + the routed call
#   repaired_one / repaired_half   (b) with one head / half of the checked heads over the bound
#                         (the route tables are put back before every call of stored_today, verified_today and the repaired_*
#                          arms: up to four small copy_ launches that are part of those arms alike)
#   verified_today        the routed call with today's fidelity sink alone (what (b) adds beyond it is the kernel + the repair launch)
#   empty_repair_launch   the dense launch over a head list with a device count of 0, alone
#   route_repair_alone    vorta_route_repair alone on a record that is already there
# and the largest launched rel_error over the heads after the repair (the routed output against dense attention on the rows).
#
# Configurations: hunyuan-129f (fp16, 24 heads) under "native" with every head on a sparse expert (the routes of
# route_by_fidelity with a bound no candidate breaks), and wan14b-81f (bf16, 40 heads) under "auto8" with the tier routes of
# route_by_fidelity(tiers=(i8pv, fp8pv, native), max_rel_error=--bound).
#
# usage: python tools/bench_route_repair.py --config hunyuan-129f --config wan14b-81f \
#            --out profiles/route_repair_timing.json --accuracy-out profiles/route_repair_accuracy.txt
import argparse
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402  (the headline configurations)
from bench_measured_precision import _layer  # noqa: E402  (one layer of a configuration: q, k, v, geometry)
from bench_routed_fidelity import _alternate  # noqa: E402  (arms in turn, device events, medians)

SAMPLES = (512, 2048)
INF = float("inf")


def _tables_of(routes):
    from vorta_amd.routed import RepairableRoutes
    made = RepairableRoutes.from_routes(routes)
    return made, [t.clone() for t in (made.expert_ids, made.lists, made.counts)] + ([] if made.tier_index is None else [made.tier_index.clone()])


def _put_back(made, saved):
    made.expert_ids.copy_(saved[0])
    made.lists.copy_(saved[1])
    made.counts.copy_(saved[2])
    if made.tier_index is not None:
        made.tier_index.copy_(saved[3])


def run(a, config, lines):
    from vorta_amd import ops
    from vorta_amd.routed import (TIERS_OF_PRECISION, route_by_fidelity, routed_attention, routed_attention_repaired,
                                  routed_attention_tiers, sample_rows, sampled_expert_fidelity)
    cfg, dev, dt, S, H, q, k, v, geom, kw = _layer(config)
    tiered = config.startswith("wan")
    tiers = TIERS_OF_PRECISION["auto8"] if tiered else None
    route_kw = dict(max_rel_error=a.bound, tiers=tiers) if tiered else dict(max_rel_error=1e3)  # (native: every head sparse)
    report = {"config": config, "dtype": str(dt), "precision": "auto8, covers_precision" if tiered else "native", "S": S, "heads": H,
              "inputs": "white noise", "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "samples": {}}
    lines.append(f"\n==== {config}: S = {S}, {H} heads, {dt}, white noise, {report['precision']}, {report['device']}")
    out = torch.empty_like(q)
    for n in SAMPLES:
        rows = sample_rows(S, n, 0, dev)
        geom.sample_tables(kw["text_valid"], rows)  # (host work, once per table: not part of a call)
        routes = route_by_fidelity(q, k, v, geom, rows=rows, **route_kw, **kw)
        made, saved = _tables_of(routes if tiered else (routes[0], routes[1]))

        def launch_today(**more):
            _put_back(made, saved)  # (an arm that repaired leaves its repairs in the tables)
            if tiered:
                return routed_attention_tiers(q, k, v, made.routings, geom, out=out, **more, **kw)
            return routed_attention(q, k, v, made.routings["native"], geom, out=out, fp8=False, **more, **kw)

        def repaired(bound):
            _put_back(made, saved)
            return routed_attention_repaired(q, k, v, made, geom, repair_above=bound, rows=rows, out=out, fp8=False, **kw)

        def measure_and_launch():
            r = route_by_fidelity(q, k, v, geom, rows=rows, **route_kw, **kw)
            if tiered:
                return routed_attention_tiers(q, k, v, r.routings, geom, out=out, operands=r.operands, **kw)
            return routed_attention(q, k, v, r[0], geom, out=out, fp8=False, **kw)

        _, rec = repaired(INF)
        rel = rec.rel.cpu()
        checked = sorted(float(x) for x in rel[~rel.isnan()])
        one = (checked[-1] + checked[-2]) / 2 if len(checked) > 1 else INF
        half = (checked[len(checked) // 2 - 1] + checked[len(checked) // 2]) / 2 if len(checked) > 1 else INF
        empty = dict(q=q[0], k=k[0], v=v[0], scale=None, out=out[0], n_q=q.shape[2], n_kv=S + kw["text_valid"],
                     q_valid=S + kw["text_valid"], tag="repair", head_list=rec.repair_list, n_heads=H,
                     n_heads_dev=torch.zeros(1, dtype=torch.int32, device=dev))
        fid = rec.fidelity
        scratch = _tables_of(routes if tiered else (routes[0], routes[1]))[0]
        arms = {"stored_today": launch_today,
                "repaired_none": lambda: repaired(INF),
                "measure_and_launch": measure_and_launch,
                "repaired_one": lambda: repaired(one),
                "repaired_half": lambda: repaired(half),
                "verified_today": lambda: launch_today(fidelity=[], fidelity_rows=rows, fidelity_heads="all" if tiered else "sparse"),
                "empty_repair_launch": lambda: ops.attn_fwd_batch([dict(empty)]),
                "route_repair_alone": lambda: ops.route_repair(fid.sq_ref, fid.sq_err, scratch.expert_ids, scratch.tier_index,
                                                               scratch.lists, scratch.counts, exact_tier=scratch.tiers.index("native"),
                                                               repair_above=INF)}
        res = _alternate(arms, a.rounds)
        worst = {}
        for name, bound in (("none", INF), ("one", one), ("half", half)):
            _, r = repaired(bound)
            after = sampled_expert_fidelity(q, k, v, geom, rows=rows, out=out, **kw).rel_error()[:, 2].cpu()
            worst[name] = dict(repair_above=bound, repaired=int(r.repair_count), checked=int((r.state_of_head != 0).sum()),
                               largest_launched_rel_before=float(rel[~rel.isnan()].max()) if len(checked) else 0.0,
                               largest_launched_rel_after=float(after.max()))
            lines.append(f"n = {n}, repair_above {bound:.5f}: {worst[name]['repaired']} of {worst[name]['checked']} checked heads "
                         f"repaired; largest launched rel_error before {worst[name]['largest_launched_rel_before']:.5f}, after "
                         f"{worst[name]['largest_launched_rel_after']:.5f}")
        a_ms, b_ms, c_ms = (res[x]["median_ms"] for x in ("stored_today", "repaired_none", "measure_and_launch"))
        report["samples"][f"n{n}"] = dict(
            arms=res, after_repair=worst,
            repair_adds_ms=round(b_ms - a_ms, 4), measuring_adds_ms=round(c_ms - a_ms, 4),
            repair_over_measuring=round((b_ms - a_ms) / (c_ms - a_ms), 4) if c_ms > a_ms else None,
            b_cheaper_than_c=bool(b_ms < c_ms))
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", choices=sorted(bench.CONFIGS), help="repeatable; default: hunyuan-129f")
    ap.add_argument("--bound", type=float, default=0.05, help="max_rel_error of the tier routes")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--accuracy-out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_route_repair.py measures on the GPU: there is no CPU path")
    lines = ["tools/bench_route_repair.py: the largest launched rel_error over the heads (the routed output against dense attention "
             "in the input dtype on the sampled rows) before and after the repair"]
    doc = {"tool": "tools/bench_route_repair.py", "runs": []}
    for config in a.config or ["hunyuan-129f"]:
        import vorta_amd.routed as rt
        rt.set_attention_precision("auto8" if config.startswith("wan") else "native")
        doc["runs"].append(run(a, config, lines))
    text = json.dumps(doc, indent=1)
    print(text)
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if a.accuracy_out:
        with open(a.accuracy_out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
