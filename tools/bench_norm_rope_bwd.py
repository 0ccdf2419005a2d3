#!/usr/bin/env python
"""Bandwidth of the norm + RoPE backward (vorta_qk_norm_rope_bwd) next to the forward (vorta_qk_norm_rope) in one process,
on the Hunyuan-129f q tensor (24 heads, 118 800 + 256 tokens, per-head norm) and the Wan-2.1-14B-81f one (40 heads, 75 600
tokens, norm across heads), both in the projection's token-major (S, H*D) layout.  Both kernels are HBM-bound; the forward
moves one read + one write of the tensor, the backward two reads + one write (cos / sin, the weight and the dweight partials
are not counted).  Windows of `--iters` launches between two device events, forward and backward alternating, `--rounds`
times; the median window is reported.

    python tools/bench_norm_rope_bwd.py [--out profiles/norm_rope_bwd_timing.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from vorta_amd import ops


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    results = []
    for name, H, S, T, across in (("hunyuan-129f q", 24, 118800, 256, False), ("wan14b-81f q", 40, 75600, 0, True)):
        mk = lambda: torch.randn((S + T, H, 128), device=dev, dtype=dt).transpose(0, 1)  # noqa: E731
        x, g, y = mk(), mk(), mk()
        dx = torch.empty_like(g)
        w = (1 + 0.1 * torch.randn(H * 128 if across else 128, device=dev)).to(dt)
        ang = torch.randn((S, 128), device=dev)
        cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
        kw = dict(cos=cos, sin=sin, rope_tokens=S, across_heads=across)
        fns = {
            "forward": lambda: ops.qk_norm_rope(y, w, 1e-6, **kw),
            "backward": lambda: ops.qk_norm_rope_bwd(x, g, w, 1e-6, dx=dx, want_dweight=False, **kw),
            "backward_dweight": lambda: ops.qk_norm_rope_bwd(x, g, w, 1e-6, dx=dx, want_dweight=True, **kw),
        }
        for fn in fns.values():  # warm every shape the timed windows use
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(window(fn, a.iters))
        tensor_gb = x.numel() * 2 / 1e9
        row = dict(shape=name, heads=H, tokens=S + T, across_heads=across, dtype="bf16", tensor_gb=round(tensor_gb, 4),
                   iters=a.iters, rounds=a.rounds)
        for k, passes in (("forward", 2), ("backward", 3), ("backward_dweight", 3)):
            med = statistics.median(ms[k])
            row[k] = dict(ms_median=round(med, 4), ms_min=round(min(ms[k]), 4), ms_max=round(max(ms[k]), 4),
                          gb_moved=round(passes * tensor_gb, 4), tb_per_s=round(passes * tensor_gb / med, 3))
            print(f"{name} {k}: {med:.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})  "
                  f"{passes * tensor_gb / med:.2f} TB/s over {passes} passes of {tensor_gb:.3f} GB", flush=True)
        row["backward_over_forward_bandwidth"] = round(row["backward"]["tb_per_s"] / row["forward"]["tb_per_s"], 3)
        results.append(row)
        del x, g, y, dx
    doc = dict(device=torch.cuda.get_device_name(0), note="GB/s = tensor bytes moved (forward: read + write; backward: two "
               "reads + one write) over the median window; tables, weight and dweight partials not counted", results=results)
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
