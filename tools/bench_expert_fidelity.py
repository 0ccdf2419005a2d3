"""Time vorta_expert_fidelity at the sizes of a training layer, beside vorta_mix_experts_bwd on the same buffers.

    python tools/bench_expert_fidelity.py --out profiles/expert_fidelity_timing.json

Both kernels read four (H, N, 128) 16-bit tensors once and write nothing large (the three expert outputs and the mixed output
/ the output gradient), so vorta_mix_experts_bwd on the same box is the yardstick: the two take turns in one process, round by
round, each round timed with device events over `--iters` launches.  Reported: the median round per kernel, the achieved
TB/s of the four tensors read once, the ratio of the two rates, and -- for context, not a yardstick -- the torch expression for
the same statistics on the same buffers.  Sizes: Hunyuan-129f (24 heads x 119 056 rows) and Wan-14B-81f (40 heads x 75 600
rows), bf16.  A measurement needs the GPU: without one this tool fails."""
import argparse
import json
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"hunyuan-129f": (24, 118800 + 256), "wan14b-81f": (40, 75600)}


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters  # ms per call


def torch_expression(xs, mixed):
    """the statistics as a training loop would write them in torch (float32 temporaries of the buffers' size)"""
    x0 = xs[0].float()
    sq_ref, max_ref = x0.square().sum((1, 2)), x0.abs().amax((1, 2))
    errs = [(t.float() - x0) for t in (xs[1], xs[2], mixed)]
    return sq_ref, max_ref, torch.stack([d.square().sum((1, 2)) for d in errs], 1), torch.stack([d.abs().amax((1, 2)) for d in errs], 1)


def measure(name, H, N, dtype, warmup, iters, rounds):
    from vorta_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    xs = [torch.randn((H, N, 128), device=dev, generator=g, dtype=torch.float32).to(dtype) for _ in range(3)]
    mixed = ((xs[0].float() + xs[1].float() + xs[2].float()) / 3).to(dtype)
    nbytes = 4 * H * N * 128 * xs[0].element_size()
    fid = lambda: ops.expert_fidelity(xs, mixed)  # noqa: E731
    bwd = lambda: ops.mix_experts_bwd(xs, mixed)  # noqa: E731
    for _ in range(warmup):
        fid(); bwd()
    torch.cuda.synchronize()
    t_fid, t_bwd = [], []
    for _ in range(rounds):  # the two take turns: the clock and the neighbours are shared
        t_fid.append(_timed(fid, iters))
        t_bwd.append(_timed(bwd, iters))
    torch_expression(xs, mixed)
    torch.cuda.synchronize()
    t_torch = [_timed(lambda: torch_expression(xs, mixed), 1) for _ in range(3)]
    # the numbers must agree before the times mean anything
    f, ref = fid(), torch_expression(xs, mixed)
    agree = max(float(((a.double() - b.double()).abs() / b.double().abs().clamp_min(1e-30)).max())
                for a, b in zip((f.sq_ref, f.max_ref, f.sq_err, f.max_err), ref))
    med = statistics.median
    rate = lambda ms: nbytes / (ms * 1e-3) / 1e12  # noqa: E731
    return dict(config=name, heads=H, rows=N, dtype=str(dtype).replace("torch.", ""), bytes_read=nbytes,
                expert_fidelity_ms=med(t_fid), expert_fidelity_ms_rounds=t_fid, expert_fidelity_tb_s=rate(med(t_fid)),
                mix_experts_bwd_ms=med(t_bwd), mix_experts_bwd_ms_rounds=t_bwd, mix_experts_bwd_tb_s=rate(med(t_bwd)),
                rate_over_mix_experts_bwd=med(t_bwd) / med(t_fid),
                torch_expression_ms=med(t_torch), torch_expression_over_kernel=med(t_torch) / med(t_fid),
                largest_relative_difference_from_torch=agree)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--configs", nargs="*", default=list(SIZES))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows-divisor", type=int, default=1, help="shrink the rows (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_expert_fidelity needs the GPU: a time taken anywhere else says nothing")
    res = dict(device=torch.cuda.get_device_properties(0).name, warmup=args.warmup, iters=args.iters, rounds=args.rounds,
               what="four (H, N, 128) tensors read once; median of the rounds; the two kernels alternate in one process",
               results=[measure(c, SIZES[c][0], SIZES[c][1] // args.rows_divisor, torch.bfloat16, args.warmup, args.iters,
                                args.rounds) for c in args.configs])
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
