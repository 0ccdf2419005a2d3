#!/usr/bin/env python
"""Diagnostic (needs a -DVORTA_TRACE build passed through VORTA_HIP_LIB): where the fused 16-bit grid of one routed layer
leaves CUs idle -- per XCD the time its last workgroup ended, per CU the idle time before the launch ended, and the gap
between a workgroup's end and the next one's start on the same CU.

    VORTA_BUILD_SUFFIX=_trace VORTA_EXTRA_FLAGS=-DVORTA_TRACE python -m vorta_amd.build
    VORTA_HIP_LIB=vorta_amd/csrc/libvorta_hip_trace.so python tools/trace_fused_grid.py [--config hunyuan-129f] [--mix uniform]

The stamps are those of csrc/attn_fwd_diag.inc (100 MHz wall clock at workgroup entry and once a wave's output stores have
left, HW_ID and XCC_ID); they go to buffers of their own, handed to the kernel in the ws_ml field of every unsplit segment.
The layer is launched back to back on random data for --seconds first (clocks and power settle), and the last launch is
the one read."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from vorta_amd import ops
from vorta_amd.routed import HeadRouting, RoutedGeometry, routed_attention


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="hunyuan-129f", choices=sorted(bench.CONFIGS))
    ap.add_argument("--mix", default="uniform", choices=sorted(bench.MIXES))
    ap.add_argument("--layer", type=int, default=0)
    ap.add_argument("--seconds", type=float, default=2.5)
    args = ap.parse_args()
    cfg = bench.CONFIGS[args.config]
    dev = torch.device("cuda:0")
    dt = torch.float16 if cfg["dtype"] == "fp16" else torch.bfloat16
    H, T, te = cfg["heads"], cfg["text"], cfg["text_valid"]
    S = cfg["latent"][0] * cfg["latent"][1] * cfg["latent"][2]
    geom = RoutedGeometry(cfg["latent"], cfg["tile"], cfg["window"], cfg["group"], cfg["rate"], dev)
    routing = HeadRouting.from_expert_ids(bench.layer_experts(cfg, args.mix, args.layer), dev)
    gen = torch.Generator(device=dev).manual_seed(1234)
    q, k, v = (torch.randn((1, H, S + T, 128), generator=gen, device=dev, dtype=dt) for _ in range(3))
    out = torch.empty_like(q)
    if te:
        geom.sta_tables(te)

    traces = {}  # segment tag -> (workgroups, buffer): [workgroups][8][8] loop records, then [workgroups][8][2] end stamps
    launch_built = ops.attn_fwd_batch_built

    def traced(built, fuse=True):
        if fuse and len(built) > 1:
            for a, _, tag, _ in built:
                if a.n_splits == 1:
                    n_wg = ops._plan(a)[1]
                    if tag not in traces:
                        traces[tag] = (n_wg, torch.zeros(n_wg * 8 * 10, dtype=torch.int64, device=dev))
                    assert traces[tag][0] == n_wg
                    a.ws_ml = traces[tag][1].data_ptr()
        launch_built(built, fuse)

    ops.attn_fwd_batch_built = traced

    def layer():
        routed_attention(q, k, v, routing, geom, model=cfg["model"], text_len=T, text_valid=te, out=out)

    layer()
    torch.cuda.synchronize()
    t0, n = time.time(), 0
    while time.time() - t0 < args.seconds:
        layer()
        torch.cuda.synchronize()
        n += 1
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    layer()
    e1.record()
    torch.cuda.synchronize()
    print(f"{args.config} {args.mix} layer {args.layer}: {n} launches in {time.time() - t0:.1f} s, then the traced one: "
          f"{e0.elapsed_time(e1):.3f} ms for the layer (events); ticket order {'on' if getattr(ops, 'FUSED_TICKETS', 0) else 'off'}")
    start, end, key, xcc, seg = [], [], [], [], []
    for i, (tag, (n_wg, buf)) in enumerate(traces.items()):
        t = buf.cpu()
        rec, fin = t[:n_wg * 64].view(n_wg, 8, 8), t[n_wg * 64:].view(n_wg, 8, 2)
        if fin[..., 0].abs().sum().item() == 0:
            print("no end stamps: not a -DVORTA_TRACE build")
            return
        ran = fin[:, 0, 0] != 0  # (a dead head slot's workgroups leave no loop record; none on this path)
        hw = fin[ran, 0, 1]
        start.append(rec[ran, 0, 5])
        end.append(fin[ran, :, 0].max(dim=1).values)
        x = (hw >> 32) & 0xf
        key.append((x * 8 + ((hw >> 13) & 0x7)) * 16 + ((hw >> 8) & 0xf))
        xcc.append(x)
        seg.append(torch.full_like(x, i))
        print(f"segment {i} {tag}: {int(ran.sum())} workgroups, entry -> end mean {((end[-1] - start[-1]).double() / 100).mean():.0f} us")
    start, end, key, xcc, seg = (torch.cat(x) for x in (start, end, key, xcc, seg))
    t0_, t1_ = start.min().item(), end.max().item()
    span = (t1_ - t0_) / 100.0
    cus = key.unique()
    print(f"launch span {span:.1f} us (first entry -> last end), {len(start)} workgroups on {len(cus)} CUs")
    print("per XCD: last workgroup end (us after the first entry), and how long before the launch's end")
    for x in sorted(xcc.unique().tolist()):
        m = xcc == x
        last = (end[m].max().item() - t0_) / 100.0
        print(f"  XCD {x}: {int(m.sum()):5d} workgroups, last end {last:10.1f}   {span - last:8.1f} us early"
              f"   by segment {[int((m & (seg == i)).sum()) for i in range(len(traces))]}")
    idle, gaps = [], []
    for c in cus.tolist():
        m = key == c
        s_, order = start[m].sort()
        e_ = end[m][order]
        idle.append((t1_ - e_.max().item()) / 100.0)
        if len(s_) > 1:
            gaps += ((s_[1:] - e_[:-1]).double() / 100.0).tolist()
    idle = torch.tensor(idle, dtype=torch.float64)
    print(f"per CU: idle before the launch's end: mean {idle.mean():.1f} us, median {idle.median():.1f}, max {idle.max():.1f}; "
          f"sum {idle.sum():.0f} us = {100 * idle.sum().item() / (span * len(cus)):.3f} % of span x CUs")
    for x in sorted(xcc.unique().tolist()):
        cm = torch.tensor([(c >> 7) == x for c in cus.tolist()])
        print(f"  XCD {x}: {int(cm.sum())} CUs, end idle mean {idle[cm].mean():.1f} us, max {idle[cm].max():.1f}")
    g = torch.tensor(gaps, dtype=torch.float64)
    print(f"gap workgroup end -> next entry on the same CU: mean {g.mean():.2f} us, median {g.median():.2f}, max {g.max():.1f}, "
          f"n = {len(gaps)}; sum {g.sum():.0f} us = {100 * g.sum().item() / (span * len(cus)):.3f} % of span x CUs")
    first = ((start - t0_).double() / 100.0).sort().values
    print(f"first-round entries within {first[len(cus) - 1]:.1f} us")


if __name__ == "__main__":
    main()
