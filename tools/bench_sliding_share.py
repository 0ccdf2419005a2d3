# What does keeping the FEWEST key tiles that hold a mass share cost, and what does it give?  (RoutedGeometry(sliding_keys=
# "share", mass_share=p): ops.sta_tile_mass, ops.sta_select_tiles_share, ops.attn_fwd_varlen)
#
# timing: one layer of a headline shape, N heads on the sliding-tile expert and no other head anywhere (hunyuan-129f: 8 of 24,
# wan14b-81f: 13 of 40), in one process with the arms alternating over --rounds rounds (device events around every call;
# median, min, max), on white-noise inputs (flat mass rows: every tile keeps the window's count, the worst case) and on
# local heads of tests/_structured_inputs.py (peaked rows):
#   window_merged          the sliding expert as the default launches it: the merged window launch, 256-row workgroups
#                          (+ Hunyuan's text-query launch, in every arm)
#   share_select_p         the selection alone at share p: the tile-mass launches + the share selection and its order
#   share_p                the same heads under sliding_keys="share": selection + the variable-length launch
#   table_full / varlen_full   the price of the new body by itself: the existing table launch and the variable-length launch
#                          over the SAME mass-chosen lists, every length n_kv (no order table); the margin is the run's own
#                          min-max spread
# with the mean and largest kept tile count per p, and the ratios to window_merged.
# --precision i8pv: every arm under the int8-score precision (the selection arms are unchanged code: they read the 16-bit q, k);
# table_full / varlen_full are then vorta_attn_fwd_i8 and vorta_attn_fwd_varlen_i8 over the operands of prepare_operands.
# accuracy: the structured families (local, redundant, white), every head on the sliding expert: per head rel_error =
# |out - dense| / |dense| over the video rows, for the window and for share at every p, with the mean kept tile count.
#
# usage: python tools/bench_sliding_share.py timing --config hunyuan-129f --config wan14b-81f --out profiles/share_tiles_timing.json
#        python tools/bench_sliding_share.py accuracy --config hunyuan-129f --config wan14b-81f --out profiles/share_tiles_accuracy.txt
#        ... --precision i8pv --out profiles/share_tiles_i8_timing.json / profiles/share_tiles_i8_accuracy.txt
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
from bench_content_tiles import FAMILIES, SLIDING_HEADS  # noqa: E402
from bench_measured_precision import _layer  # noqa: E402  (one layer of a configuration: q, k, v, geometry)
from bench_routed_fidelity import _alternate  # noqa: E402  (arms in turn, device events, medians)

SHARES = (0.90, 0.95, 0.99)


def _geom(cfg, dev, **kw):
    from vorta_amd.routed import RoutedGeometry
    return RoutedGeometry(cfg["latent"], cfg["tile"], cfg["window"], cfg["group"], cfg["rate"], dev, **kw)


def timing_of(a, config, inputs):
    import _structured_inputs as SI
    from vorta_amd import ops
    from vorta_amd.routed import MASS_ROWS_PER_TILE, HeadRouting, prepare_operands, routed_attention
    cfg, dev, dt, S, H, q, k, v, window, kw = _layer(config)
    fp8 = False if a.precision == "native" else a.precision
    n = SLIDING_HEADS.get(config, max(1, H // 3))
    te = kw["text_valid"]
    if inputs == "local":  # the video rows of the sliding heads become local heads; the text rows stay white
        gen = torch.Generator(device=dev).manual_seed(11)
        for h in range(n):
            for x, y in zip((q, k, v), SI.local_head(cfg["latent"], (2.0, 3.0, 4.0), 16.0, 0.05, gen, dev)):
                x[0, h, :S] = y.to(dt)
    routing = HeadRouting.from_expert_ids([2] * n + [-1] * (H - n), dev)  # (a head with no expert is in no list)
    slots = routing.slot_args(2, H)
    out = torch.empty_like(q)
    geoms = {p: _geom(cfg, dev, sliding_keys="share", mass_share=p) for p in SHARES}
    q_rows, _, n_kv = geoms[SHARES[0]].sta_tables(te)
    n_tiles, tok, _ = ops.sta_table_sizes(cfg["latent"], cfg["tile"], cfg["window"], te)
    arms = {"window_merged": lambda: routed_attention(q, k, v, routing, window, out=out, fp8=fp8, **kw)}
    tabs = {}
    for p, g in geoms.items():
        g.prebuild(te, content_slots=n)
        tabs[p] = g.share_buffers(te, n, 256)

        def select(p=p, g=g):
            ops.sta_tile_mass(q[0], k[0], g.latent, g.tile, g.window, te, q_rows, tabs[p].ws, scale=kw.get("scale"),
                              rows_per_tile=MASS_ROWS_PER_TILE, **slots)
            ops.sta_select_tiles_share(g.latent, g.tile, g.window, te, q_rows, tabs[p], mass_share=p, n_heads=slots["n_heads"],
                                       rows_per_tile=MASS_ROWS_PER_TILE, n_heads_dev=slots.get("n_heads_dev"))
        arms[f"share_select_{p}"] = select
        arms[f"share_{p}"] = lambda g=g: routed_attention(q, k, v, routing, g, out=out, fp8=fp8, **kw)
    # the body alone: the same full-length lists through the existing table launch and through the variable-length one
    mass = _geom(cfg, dev, sliding_keys="mass")
    kv_rows, _, _ = ops.sta_select_tiles(q[0], k[0], mass.latent, mass.tile, mass.window, te, q_rows, scores="mass",
                                         scale=kw.get("scale"), rows_per_tile=MASS_ROWS_PER_TILE, **slots)
    full = torch.full((n, n_tiles), n_kv, dtype=torch.int32, device=dev)
    launch = dict(n_q=S, q_group_len=tok, n_kv=n_kv, q_rows=q_rows, kv_rows=kv_rows, kv_rows_stride_g=kv_rows.stride(1),
                  block_rows=256, **slots)
    operands = prepare_operands(a.precision, q[0], k[0], v[0], kw.get("scale")).kwargs(kw.get("scale"))
    arms["table_full"] = lambda: ops.attn_fwd(out=out[0], **operands, **launch)
    arms["varlen_full"] = lambda: ops.attn_fwd_varlen(out=out[0], kv_len=full, **operands, **launch)
    res = _alternate(arms, a.rounds)
    torch.cuda.synchronize()
    counts = {str(p): {"mean": round(float(tabs[p].sel_count.float().mean()), 3), "max": int(tabs[p].sel_count.max())} for p in SHARES}
    base, tab = res["window_merged"]["median_ms"], res["table_full"]
    return {"config": config, "inputs": inputs, "precision": a.precision, "dtype": str(dt), "S": S, "heads": H, "sliding_heads": n, "n_tiles": n_tiles,
            "tok": tok, "n_kv": n_kv, "n_sel": (n_kv - te) // tok, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
            "arms": res, "kept_tiles": counts,
            "ratio_to_window_merged": {name: round(res[name]["median_ms"] / base, 4) for name in res if name.startswith("share_0")},
            "varlen_full_over_table_full": round(res["varlen_full"]["median_ms"] / tab["median_ms"], 4),
            "table_full_spread": round((tab["max_ms"] - tab["min_ms"]) / tab["median_ms"], 4)}


def accuracy_of(a, config, lines):
    import _structured_inputs as SI
    from vorta_amd.routed import HeadRouting, routed_attention
    cfg = bench.CONFIGS[config]
    dev, dt = torch.device("cuda:0"), torch.float16 if cfg["dtype"] == "fp16" else torch.bfloat16
    latent, S = cfg["latent"], cfg["latent"][0] * cfg["latent"][1] * cfg["latent"][2]
    geoms = {"window": _geom(cfg, dev, sliding_keys="window")}
    geoms.update({p: _geom(cfg, dev, sliding_keys="share", mass_share=p) for p in SHARES})
    lines.append(f"\n==== {config}: S = {S}, {dt}, every head on the sliding-tile expert, {torch.cuda.get_device_name(0)}")
    for noise in a.noise:
        gen = torch.Generator(device=dev).manual_seed(11)
        q, k, v = (x.to(dt) for x in SI.structured_layer(latent, [2, 1, 0], cfg["tile"], cfg["group"], noise, gen, dev))
        kw = dict(model="wan", fp8=False)  # (video tokens alone: the families have no text part)
        dense = routed_attention(q, k, v, HeadRouting.from_expert_ids([0, 0, 0], dev), geoms["window"], **kw).float()
        kw["fp8"] = False if a.precision == "native" else a.precision  # (the dense reference stays in the input dtype)
        rel, kept = {}, {}
        for name, geom in geoms.items():
            o = routed_attention(q, k, v, HeadRouting.from_expert_ids([2, 2, 2], dev), geom, **kw).float()
            rel[name] = ((o - dense)[0].flatten(1).norm(dim=1) / dense[0].flatten(1).norm(dim=1)).tolist()
            if name != "window":
                kept[name] = geom.share_buffers(0, 3, 256).sel_count.float().mean(1).tolist()
        n_sel = geoms[SHARES[0]].share_buffers(0, 3, 256).sel_tiles.shape[2]
        for h, fam in enumerate(FAMILIES):
            lines.append(f"noise {noise}: {a.precision} {fam:9s} head: rel_error window {rel['window'][h]:.5f} ({n_sel} tiles)  " +
                         "  ".join(f"share {p}: {rel[p][h]:.5f} ({kept[p][h]:.2f} tiles)" for p in SHARES))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["timing", "accuracy"])
    ap.add_argument("--config", action="append", choices=sorted(bench.CONFIGS), help="repeatable; default: hunyuan-129f")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--precision", choices=["native", "i8pv"], default="native", help="the precision of every attention launch")
    ap.add_argument("--noise", type=float, action="append", help="accuracy: white-noise share of the structured heads; repeatable")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    a.noise = a.noise or [0.05, 0.3]
    if not torch.cuda.is_available():
        raise SystemExit("bench_sliding_share.py measures on the GPU: there is no CPU path")
    configs = a.config or ["hunyuan-129f"]
    if a.what == "timing":
        runs = [timing_of(a, c, inputs) for c in configs for inputs in ("white", "local")]
        text = json.dumps({"tool": "tools/bench_sliding_share.py timing", "runs": runs}, indent=1)
    else:
        lines = ["tools/bench_sliding_share.py accuracy: per-head rel_error of the sliding-tile expert against dense attention "
                 "(|out - dense| / |dense| over the video rows), window key tiles and the fewest mass-ranked tiles that hold a "
                 "share p of the sampled mass (mean kept tiles per query tile in brackets)"]
        for c in configs:
            accuracy_of(a, c, lines)
        text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
