"""Forward and backward time of the gather attention at model size (recorded, not gated; bench.py is the project's yardstick
and is not involved).

    python tools/bench_attn_bwd.py --case dense   --config hunyuan-129f     one dense head
    python tools/bench_attn_bwd.py --case mixture --config wan1.3b-49f      the full soft-mixture layer, every head
    python tools/bench_attn_bwd.py --all --out profiles/attn_bwd_timing.json

`--all` runs the four (case, config) steps as child processes, each under its own `timeout -k 10`, in a chain that stops at
the first step that fails (the shell form: `timeout -k 10 600 python tools/bench_attn_bwd.py --case dense --config
hunyuan-129f && timeout -k 10 600 ...`), and collects their JSON lines.  The yardstick of the backward figure is the forward of
the SAME launches in the same process; FLOPs count the five products of the backward plus the recomputed scores (6 / 2 of
the forward's 4 S_q S_kv D per head)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("dense", "hunyuan-129f"), ("dense", "wan1.3b-49f"), ("mixture", "hunyuan-129f"), ("mixture", "wan1.3b-49f")]


def _time(fn, warmup, steps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def run_one(case, config, warmup, steps):
    import torch
    from bench import CONFIGS
    from vorta_amd import ops, routed
    cfg = CONFIGS[config]
    dev = torch.device("cuda:0")
    dtype = torch.float16 if cfg["dtype"] == "fp16" else torch.bfloat16
    S = cfg["latent"][0] * cfg["latent"][1] * cfg["latent"][2]
    T, te = cfg["text"], cfg["text_valid"]
    H = 1 if case == "dense" else cfg["heads"]
    gen = torch.Generator(device="cpu").manual_seed(0)
    q, k, v, g = (torch.randn((1, H, S + T, 128), generator=gen, dtype=torch.float32).to(dtype).to(dev) for _ in range(4))
    launches = []
    if case == "dense":
        out = torch.empty_like(q)
        launches = [dict(q=q[0], k=k[0], v=v[0], out=out[0], n_q=S + T, n_kv=S + te, q_valid=S + te,
                         flops=4.0 * (S + te) ** 2 * 128)]
        weight_of = None
        fwd = lambda: ops.attn_fwd_batch(launches)  # noqa: E731
    else:
        geom = routed.geometry_for(cfg["latent"], cfg["tile"], cfg["window"], cfg["group"], cfg["rate"], dev)
        bufs = [torch.empty_like(q) for _ in range(3)]
        sc = torch.softmax(torch.randn((1, H, 3), generator=gen), dim=-1).to(dtype).to(dev)
        routing = routed.HeadRouting.every_head_everywhere(H, dev)
        kw = dict(model=cfg["model"], text_len=T, text_valid=te, expert_outs=bufs, fp8=False)
        routed.routed_attention(q, k, v, routing, geom, record=launches, **kw)
        s16 = sc[0].contiguous()
        weight_of = lambda c, o: s16[:, next(i for i, b in enumerate(bufs) if b.data_ptr() == o.data_ptr())]  # noqa: E731
        fwd = lambda: routed.routed_attention(q, k, v, routing, geom, **kw)  # noqa: E731
    acc = [torch.zeros(q.shape[1:], dtype=torch.float32, device=dev) for _ in range(3)]
    bwd = lambda: routed._replay_backward(launches, g[0], acc[0], acc[1], acc[2], weight_of)  # noqa: E731
    fwd_ms = _time(fwd, warmup, steps)
    bwd_ms = _time(bwd, warmup, steps)
    fwd_flops = sum(c.get("flops", 0.0) for c in launches)
    return dict(case=case, config=config, dtype=cfg["dtype"], heads=H, tokens=S + T, launches=len(launches),
                warmup=warmup, steps=steps, fwd_ms=round(fwd_ms, 3), bwd_ms=round(bwd_ms, 3),
                bwd_over_fwd=round(bwd_ms / fwd_ms, 3), fwd_tflops=round(fwd_flops / fwd_ms / 1e9, 1),
                bwd_tflops=round(3.0 * fwd_flops / bwd_ms / 1e9, 1), device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["dense", "mixture"])
    ap.add_argument("--config", default="hunyuan-129f")
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=280)
    a = ap.parse_args()
    if not a.all:
        print(json.dumps(run_one(a.case, a.config, a.warmup, a.steps)), flush=True)
        return 0
    results = []
    for case, config in STEPS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--case", case,
               "--config", config, "--warmup", str(a.warmup), "--steps", str(a.steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:  # nothing more is started on the GPU after a step that failed
            print(r.stdout[-2000:], r.stderr[-2000:], f"step {case} {config} ended with {r.returncode}: stopping", sep="\n")
            return r.returncode
        line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
        print(line, flush=True)
        results.append(json.loads(line))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(note="backward / forward of the same launches in one process; TFLOP/s count 4 S_q S_kv D per head "
                                "and launch for the forward and 3 x that (5 products + the recomputed scores) for the backward",
                           results=results), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
