# What does running the FULL-attention expert on the fewest key tiles that hold a mass share cost, and what does it give?
# (RoutedGeometry(full_keys="share", full_mass_share=p): ops.sta_tile_mass, ops.sta_select_tiles_share_all,
# ops.attn_fwd_tilelist)
#
# timing: one layer of a headline shape, N heads on the full-attention expert and no other head anywhere (a third of the heads:
# hunyuan-129f 8 of 24, wan14b-81f 13 of 40), in one process with the arms alternating over --rounds rounds (device events
# around every call; median, min, max), on white-noise inputs (flat mass rows: every list is full or nearly, the worst case) and
# on local heads of tests/_structured_inputs.py (peaked rows):
#   dense                  the heads as full_keys="all" launches them today: the baseline
#   share_select_p         the selection alone at share p: the tile-mass launches + the selection over all tiles and its order
#   share_p                the same heads under full_keys="share": selection + the tile-list launch (+ Hunyuan's text queries)
# with the mean, smallest and largest kept tile count per p, the ratios to dense and dense's own min-max spread.
# accuracy: the structured families (local, redundant, white), every head on the full expert: per head rel_error =
# |out - dense| / |dense| over the video rows at every p, with the mean kept tile count.
#
# usage: python tools/bench_full_share.py timing --config hunyuan-129f --config wan14b-81f --out profiles/full_share_timing.json
#        python tools/bench_full_share.py accuracy --config hunyuan-129f --config wan14b-81f --out profiles/full_share_accuracy.txt
import argparse
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402  (the headline configurations)
from bench_content_tiles import FAMILIES, SLIDING_HEADS as THIRD_OF_HEADS  # noqa: E402
from bench_measured_precision import _layer  # noqa: E402  (one layer of a configuration: q, k, v, geometry)
from bench_routed_fidelity import _alternate  # noqa: E402  (arms in turn, device events, medians)

SHARES = (0.90, 0.95, 0.99)


def _geom(cfg, dev, **kw):
    from vorta_amd.routed import RoutedGeometry
    return RoutedGeometry(cfg["latent"], cfg["tile"], cfg["window"], cfg["group"], cfg["rate"], dev, **kw)


def timing_of(a, config, inputs):
    import _structured_inputs as SI
    from vorta_amd import ops
    from vorta_amd.routed import MASS_ROWS_PER_TILE, HeadRouting, _tile_block_rows, routed_attention
    cfg, dev, dt, S, H, q, k, v, dense_geom, kw = _layer(config)
    n = THIRD_OF_HEADS.get(config, max(1, H // 3))
    te = kw["text_valid"]
    if inputs == "local":  # the video rows of the full heads become local heads; the text rows stay white
        gen = torch.Generator(device=dev).manual_seed(11)
        for h in range(n):
            for x, y in zip((q, k, v), SI.local_head(cfg["latent"], (2.0, 3.0, 4.0), 16.0, 0.05, gen, dev)):
                x[0, h, :S] = y.to(dt)
    routing = HeadRouting.from_expert_ids([0] * n + [-1] * (H - n), dev)  # (a head with no expert is in no list)
    slots = routing.slot_args(0, H)
    out = torch.empty_like(q)
    geoms = {p: _geom(cfg, dev, full_keys="share", full_mass_share=p) for p in SHARES}
    q_rows = geoms[SHARES[0]].sta_tables(te)[0]
    arms = {"dense": lambda: routed_attention(q, k, v, routing, dense_geom, out=out, fp8=False, **kw)}
    tabs = {}
    for p, g in geoms.items():
        g.sta_tables(te)
        tabs[p] = g.full_share_buffers(n)

        def select(p=p, g=g):
            ops.sta_tile_mass(q[0], k[0], g.latent, g.tile, g.window, te, q_rows, tabs[p].ws, scale=kw.get("scale"),
                              rows_per_tile=MASS_ROWS_PER_TILE, **slots)
            ops.sta_select_tiles_share_all(g.latent, g.tile, te, tabs[p], mass_share=p, n_heads=slots["n_heads"],
                                           rows_per_tile=MASS_ROWS_PER_TILE, block_rows=_tile_block_rows(g.tok),
                                           n_heads_dev=slots.get("n_heads_dev"))
        arms[f"share_select_{p}"] = select
        arms[f"share_{p}"] = lambda g=g: routed_attention(q, k, v, routing, g, out=out, fp8=False, **kw)
    res = _alternate(arms, a.rounds)
    torch.cuda.synchronize()
    n_tiles = tabs[SHARES[0]].sel_tiles.shape[1]
    counts = {str(p): {"mean": round(float(tabs[p].sel_count.float().mean()), 3), "min": int(tabs[p].sel_count.min()),
                       "max": int(tabs[p].sel_count.max())} for p in SHARES}
    base = res["dense"]
    return {"config": config, "inputs": inputs, "dtype": str(dt), "S": S, "heads": H, "full_heads": n, "n_tiles": n_tiles,
            "tok": geoms[SHARES[0]].tok, "block_rows": _tile_block_rows(geoms[SHARES[0]].tok), "rounds": a.rounds,
            "device": torch.cuda.get_device_name(0), "arms": res, "kept_tiles": counts,
            "ratio_to_dense": {name: round(res[name]["median_ms"] / base["median_ms"], 4) for name in res if name != "dense"},
            "dense_spread": round((base["max_ms"] - base["min_ms"]) / base["median_ms"], 4)}


def accuracy_of(a, config, lines):
    import _structured_inputs as SI
    from vorta_amd.routed import HeadRouting, routed_attention
    cfg = bench.CONFIGS[config]
    dev, dt = torch.device("cuda:0"), torch.float16 if cfg["dtype"] == "fp16" else torch.bfloat16
    latent, S = cfg["latent"], cfg["latent"][0] * cfg["latent"][1] * cfg["latent"][2]
    geoms = {p: _geom(cfg, dev, full_keys="share", full_mass_share=p) for p in SHARES}
    routing = HeadRouting.from_expert_ids([0, 0, 0], dev)
    lines.append(f"\n==== {config}: S = {S}, {dt}, every head on the full-attention expert, {torch.cuda.get_device_name(0)}")
    for noise in a.noise:
        gen = torch.Generator(device=dev).manual_seed(11)
        q, k, v = (x.to(dt) for x in SI.structured_layer(latent, [2, 1, 0], cfg["tile"], cfg["group"], noise, gen, dev))
        kw = dict(model="wan", fp8=False)  # (video tokens alone: the families have no text part)
        dense = routed_attention(q, k, v, routing, _geom(cfg, dev, full_keys="all"), **kw).float()
        rel, kept = {}, {}
        for p, geom in geoms.items():
            o = routed_attention(q, k, v, routing, geom, **kw).float()
            rel[p] = ((o - dense)[0].flatten(1).norm(dim=1) / dense[0].flatten(1).norm(dim=1)).tolist()
            kept[p] = geom.full_share_buffers(3).sel_count.float().mean(1).tolist()
        n_tiles = geoms[SHARES[0]].full_share_buffers(3).sel_tiles.shape[1]
        for h, fam in enumerate(FAMILIES):
            lines.append(f"noise {noise}: {fam:9s} head, {n_tiles} tiles: " +
                         "  ".join(f"share {p}: rel_error {rel[p][h]:.5f} ({kept[p][h]:.2f} tiles)" for p in SHARES))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["timing", "accuracy"])
    ap.add_argument("--config", action="append", choices=sorted(bench.CONFIGS), help="repeatable; default: hunyuan-129f")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--noise", type=float, action="append", help="accuracy: white-noise share of the structured heads; repeatable")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    a.noise = a.noise or [0.05, 0.3]
    if not torch.cuda.is_available():
        raise SystemExit("bench_full_share.py measures on the GPU: there is no CPU path")
    configs = a.config or ["hunyuan-129f"]
    if a.what == "timing":
        runs = [timing_of(a, c, inputs) for c in configs for inputs in ("white", "local")]
        text = json.dumps({"tool": "tools/bench_full_share.py timing", "runs": runs}, indent=1)
    else:
        lines = ["tools/bench_full_share.py accuracy: per-head rel_error of the full-attention expert under full_keys='share' against "
                 "dense attention (|out - dense| / |dense| over the video rows): the fewest mass-ranked tiles, out of all, that "
                 "hold a share p of the sampled mass (mean kept tiles per query tile in brackets)"]
        for c in configs:
            accuracy_of(a, c, lines)
        text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
