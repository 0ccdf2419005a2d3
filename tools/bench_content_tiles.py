# What do content-chosen key tiles cost, and what do they give?  (ops.sta_select_tiles, vorta_sta_select_tiles,
# RoutedGeometry(sliding_keys="content"))
#
# timing: one layer of a headline shape, white-noise inputs, N heads on the sliding-tile expert and no other head anywhere
# (hunyuan-129f: 8 of 24, wan14b-81f: 13 of 40), in one process with the arms alternating over --rounds rounds (device events
# around every call; median, min, max):
#   select_both / tile_means / select_expand   the selection alone: both launches, the HBM-bound means pass, the score +
#                                              rank + expansion pass (from the means an earlier call left)
#   window_merged                  the sliding expert as the parent commit launches it: the merged window launch, 256-row
#                                  workgroups (+ Hunyuan's text-query launch, in every arm)
#   content_br256 / content_br128  the same heads with content lists: selection + the un-merged launch (a tile is a group)
#   content_launch_br256 / _br128  that launch alone, over lists already selected
#   mass_scores / mass_select      the mass statistic alone (ops.sta_tile_mass: the MFMA scoring launch + the reduction), and
#                                  the whole mass selection (those two + the rank and expansion from its matrix)
#   mass_br256 / mass_br128        the same heads under sliding_keys="mass": mass selection + the un-merged launch
# and the ratios of the content and mass arms to window_merged.
# accuracy: the structured families of tests/_structured_inputs.py (local, redundant, white), every head on the sliding
# expert: per head rel_error = |out - dense| / |dense| over the video rows, for window, content and mass lists.
#
# usage: python tools/bench_content_tiles.py timing --config hunyuan-129f --config wan14b-81f --out profiles/content_tiles_timing.json
#        python tools/bench_content_tiles.py accuracy --config hunyuan-129f --config wan14b-81f --out profiles/content_tiles_accuracy.txt
#        (with the mass arms: profiles/mass_tiles_timing.json, profiles/mass_tiles_accuracy.txt)
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
from bench_measured_precision import _layer  # noqa: E402  (one layer of a configuration: q, k, v, geometry)
from bench_routed_fidelity import _alternate  # noqa: E402  (arms in turn, device events, medians)

SLIDING_HEADS = {"hunyuan-129f": 8, "wan14b-81f": 13}
FAMILIES = ("local", "redundant", "white")  # structured_layer's kinds by the expert a head is built for: 2, 1, 0


def timing_of(a, config):
    from vorta_amd import ops
    from vorta_amd.routed import HeadRouting, RoutedGeometry, routed_attention
    cfg, dev, dt, S, H, q, k, v, window, kw = _layer(config)
    n = SLIDING_HEADS.get(config, max(1, H // 3))
    content = RoutedGeometry(cfg["latent"], cfg["tile"], cfg["window"], cfg["group"], cfg["rate"], dev, sliding_keys="content")
    te = kw["text_valid"]
    content.prebuild(te, content_slots=n)
    routing = HeadRouting.from_expert_ids([2] * n + [-1] * (H - n), dev)  # (a head with no expert is in no list)
    out = torch.empty_like(q)
    q_rows, _, n_kv = content.sta_tables(te)
    slots = routing.slot_args(2, H)
    bufs = content.content_buffers(te, n)
    select = lambda phases: ops.sta_select_tiles(q[0], k[0], cfg["latent"], cfg["tile"], cfg["window"], te, q_rows, out=bufs,  # noqa: E731
                                                 phases=phases, **slots)
    from vorta_amd.routed import MASS_ROWS_PER_TILE
    mass = RoutedGeometry(cfg["latent"], cfg["tile"], cfg["window"], cfg["group"], cfg["rate"], dev, sliding_keys="mass")
    mass.prebuild(te, content_slots=n)
    mbufs = mass.content_buffers(te, n)
    mass_kw = dict(scale=kw.get("scale"), rows_per_tile=MASS_ROWS_PER_TILE)
    launches = {}
    for br in (256, 128):
        rec = []
        routed_attention(q, k, v, routing, content, out=out, fp8=False, sliding_block_rows=br, record=rec, **kw)
        launches[br] = rec  # (a recorded call keeps lists of its own)
    arms = {"select_both": lambda: select(0), "tile_means": lambda: select(1), "select_expand": lambda: select(2),
            "window_merged": lambda: routed_attention(q, k, v, routing, window, out=out, fp8=False, **kw)}
    arms["mass_scores"] = lambda: ops.sta_tile_mass(q[0], k[0], cfg["latent"], cfg["tile"], cfg["window"], te, q_rows, mbufs[2],
                                                    **mass_kw, **slots)
    arms["mass_select"] = lambda: ops.sta_select_tiles(q[0], k[0], cfg["latent"], cfg["tile"], cfg["window"], te, q_rows, out=mbufs,
                                                       scores="mass", **mass_kw, **slots)
    for br in (256, 128):
        arms[f"mass_br{br}"] = lambda br=br: routed_attention(q, k, v, routing, mass, out=out, fp8=False,
                                                              sliding_block_rows=br, **kw)
        arms[f"content_br{br}"] = lambda br=br: routed_attention(q, k, v, routing, content, out=out, fp8=False,
                                                                 sliding_block_rows=br, **kw)
        arms[f"content_launch_br{br}"] = lambda br=br: ops.attn_fwd_batch([dict(c) for c in launches[br]])
    res = _alternate(arms, a.rounds)
    base = res["window_merged"]["median_ms"]
    n_tiles, tok, _ = ops.sta_table_sizes(cfg["latent"], cfg["tile"], cfg["window"], te)
    return {"config": config, "dtype": str(dt), "S": S, "heads": H, "sliding_heads": n, "n_tiles": n_tiles, "tok": tok, "n_kv": n_kv,
            "inputs": "white noise", "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "arms": res,
            "bytes": {"tile_means_read": 2 * n * S * 128 * q.element_size(), "key_lists_written": n * n_tiles * n_kv * 4,
                      "mass_pairs_written": n * n_tiles * MASS_ROWS_PER_TILE * n_tiles * 8},
            "mass_rows_per_tile": MASS_ROWS_PER_TILE, "mass_score_flop": 2.0 * n * n_tiles * MASS_ROWS_PER_TILE * S * 128,
            "ratio_to_window_merged": {name: round(res[name]["median_ms"] / base, 4) for name in res
                                       if name.startswith(("content", "mass_br"))}}


def accuracy_of(a, config, lines):
    import _structured_inputs as SI
    from vorta_amd.routed import HeadRouting, RoutedGeometry, routed_attention
    cfg = bench.CONFIGS[config]
    dev, dt = torch.device("cuda:0"), torch.float16 if cfg["dtype"] == "fp16" else torch.bfloat16
    latent, S = cfg["latent"], cfg["latent"][0] * cfg["latent"][1] * cfg["latent"][2]
    geoms = {name: RoutedGeometry(latent, cfg["tile"], cfg["window"], cfg["group"], cfg["rate"], dev, sliding_keys=name)
             for name in ("window", "content", "mass")}
    lines.append(f"\n==== {config}: S = {S}, {dt}, every head on the sliding-tile expert, {torch.cuda.get_device_name(0)}")
    for noise in a.noise:
        gen = torch.Generator(device=dev).manual_seed(11)
        q, k, v = (x.to(dt) for x in SI.structured_layer(latent, [2, 1, 0], cfg["tile"], cfg["group"], noise, gen, dev))
        kw = dict(model="wan", fp8=False)  # (video tokens alone: the families have no text part)
        dense = routed_attention(q, k, v, HeadRouting.from_expert_ids([0, 0, 0], dev), geoms["window"], **kw).float()
        rel = {}
        for name, geom in geoms.items():
            out = routed_attention(q, k, v, HeadRouting.from_expert_ids([2, 2, 2], dev), geom, **kw).float()
            rel[name] = ((out - dense)[0].flatten(1).norm(dim=1) / dense[0].flatten(1).norm(dim=1)).tolist()
        for h, fam in enumerate(FAMILIES):
            w, c, m = rel["window"][h], rel["content"][h], rel["mass"][h]
            lines.append(f"noise {noise}: {fam:9s} head: rel_error window {w:.5f} content {c:.5f} mass {m:.5f}  "
                         f"({'content better' if c < w else 'content worse' if c > w else 'equal'}; "
                         f"{'mass better' if m < w else 'mass worse' if m > w else 'mass equal'})")


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
        raise SystemExit("bench_content_tiles.py measures on the GPU: there is no CPU path")
    configs = a.config or ["hunyuan-129f"]
    if a.what == "timing":
        text = json.dumps({"tool": "tools/bench_content_tiles.py timing", "runs": [timing_of(a, c) for c in configs]}, indent=1)
    else:
        lines = ["tools/bench_content_tiles.py accuracy: per-head rel_error of the sliding-tile expert against dense attention "
                 "(|out - dense| / |dense| over the video rows), window key tiles, content-chosen key tiles (tile means) and "
                 "mass-chosen key tiles (sampled attention mass)"]
        for c in configs:
            accuracy_of(a, c, lines)
        text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
