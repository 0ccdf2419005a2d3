"""One routed layer at Hunyuan-129f under the geometry bench.py runs and under the published one (recorded, not gated;
bench.py is the project's yardstick and is not involved).

    python tools/bench_partial_geometry.py --out profiles/partial_geometry_timing.json

fp16, latent (33,45,80), 24 heads with 8 / 8 / 8 on the full / coreset / sliding-tile expert, text 256 with 96 valid.
"proposed": tile (11,9,8), coreset window (3,3,2) -- divides the grid, the sliding expert sees every frame.
"published": tile (6,9,8), coreset window (2,3,2) -- the authors' checkpoint geometry, which does not divide 33 frames and
runs only with partial geometry switched on (DESIGN.md "Partial geometry").
One process; the two geometries take turns over ROUNDS rounds (a drift of the clock shows in both); every figure is device
events around warmed launches: the fused layer (`layer_ms`), and from unfused runs under ops.Timeline the launches of each
expert (`launch_ms`, summed per tag).  Key counts and S_low come from the geometry objects."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LATENT, WINDOW, HEADS, TEXT, TEXT_VALID = (33, 45, 80), (3, 3, 3), 24, 256, 96
GEOMETRIES = {"proposed": dict(tile=(11, 9, 8), group=(3, 3, 2)), "published": dict(tile=(6, 9, 8), group=(2, 3, 2))}
ROUNDS = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import vorta_amd
    from vorta_amd import ops, routed
    vorta_amd.set_partial_geometry(True)
    dev, dtype = torch.device("cuda:0"), torch.float16
    S = LATENT[0] * LATENT[1] * LATENT[2]
    gen = torch.Generator(device="cpu").manual_seed(0)
    q, k, v = (torch.randn((1, HEADS, S + TEXT, 128), generator=gen).to(dtype).to(dev) for _ in range(3))
    out = torch.empty_like(q)
    routing = routed.HeadRouting.from_expert_ids([h % 3 for h in range(HEADS)], dev)
    kw = dict(model="hunyuan", text_len=TEXT, text_valid=TEXT_VALID, out=out, fp8=False)
    geoms = {n: routed.geometry_for(LATENT, g["tile"], WINDOW, g["group"], 0.5, dev) for n, g in GEOMETRIES.items()}
    res = {}
    for n, g in geoms.items():
        g.prebuild(TEXT_VALID)
        res[n] = dict(GEOMETRIES[n], partial=g.is_partial, S_low=g.S_low, G=g.G, C=g.C, sliding_video_keys=g.sta_class_n_kv,
                      layer_ms_rounds=[], launch_ms_rounds=[])

    def timed(fn, steps):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    for _ in range(ROUNDS):
        for n, g in geoms.items():
            res[n]["layer_ms_rounds"].append(round(timed(lambda: routed.routed_attention(q, k, v, routing, g, **kw), args.steps), 3))
            unfused = lambda: routed.routed_attention(q, k, v, routing, g, fused=False, sliding_block_rows=256, **kw)  # noqa: E731
            for _ in range(args.warmup):
                unfused()
            tl = ops.Timeline()
            ops.set_timeline(tl)
            try:
                for _ in range(args.steps):
                    unfused()
            finally:
                ops.set_timeline(None)
            per = {}
            for (tag, _), d in tl.summary().items():
                per[tag] = round(per.get(tag, 0.0) + d["ms"] / args.steps, 3)
            res[n]["launch_ms_rounds"].append(per)
    for n in res:
        r = res[n]
        r["layer_ms"] = round(sum(r["layer_ms_rounds"]) / ROUNDS, 3)
        r["launch_ms"] = {t: round(sum(p[t] for p in r["launch_ms_rounds"]) / ROUNDS, 3) for t in r["launch_ms_rounds"][0]}
    a, b = res["proposed"], res["published"]
    line = dict(what="one routed layer, Hunyuan-129f fp16, 8/8/8 heads, text 256/96; device events, one process, alternating",
                device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, rounds=ROUNDS, geometries=res,
                sliding_ms_ratio_published_over_proposed=round(b["launch_ms"]["sliding"] / a["launch_ms"]["sliding"], 3),
                layer_ms_ratio_published_over_proposed=round(b["layer_ms"] / a["layer_ms"], 3))
    print(json.dumps(line))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
