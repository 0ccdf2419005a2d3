#!/usr/bin/env python3
"""One layer of the soft mixture, forward + backward, under sequence parallelism: two gloo ranks SHARING one GPU, beside the
single-GPU operator on the whole sequence.

    python tools/bench_sp_soft_mixture.py --out profiles/sp_soft_mixture_timing.json

A record, not a gate.  Ranks that share a GPU say nothing about a wire: the exchange is staged through the host (gloo cannot
move device memory) and the two ranks' kernels compete for the same CUs, so `sp_ms` is NOT what two GPUs would take.  Nobody
has measured this exchange between GPUs.  What the figure does show: the whole path runs at these sizes, and what the
host-staged rehearsal costs."""
import argparse
import json
import os
import socket
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    # the shape of tests/test_hip_sp_soft_mixture.py
    "test": dict(model="hunyuan", latent=(12, 6, 8), tile=(2, 3, 4), window=(3, 3, 3), group=(2, 3, 2), rate=0.5, heads=4,
                 text=8, text_valid=5),
    # bench.py CONFIGS["wan1.3b-49f"]
    "wan1.3b-49f": dict(model="wan", latent=(13, 20, 32), tile=(13, 10, 8), window=(3, 3, 3), group=(1, 2, 2), rate=0.5,
                        heads=12, text=0, text_valid=0),
}


def _inputs(cfg, dtype, dev):
    g = torch.Generator().manual_seed(1)
    S, T, H = cfg["latent"][0] * cfg["latent"][1] * cfg["latent"][2], cfg["text"], cfg["heads"]
    q, k, v = (torch.randn((1, H, S + T, 128), generator=g).to(dtype).to(dev) for _ in range(3))
    sc = torch.softmax(torch.randn((1, H, 3), generator=g), dim=-1).to(dtype).to(dev)
    return q, k, v, sc, S, T


def _time(step, warmup, iters):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _group_info(cfg, dev):
    from vorta_amd.attention import get_group_info
    return get_group_info(cfg["latent"], cfg["group"], cfg["rate"], dev)


def _worker(rank, world, port, ret, warmup, iters):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    from vorta_amd.routed import sp_soft_mixture_attention_autograd
    from vorta_amd.ulysses import SP_STATE
    SP_STATE.setup_sp_group(world)
    res = {}
    for name, cfg in SHAPES.items():
        q, k, v, sc, S, T = _inputs(cfg, torch.bfloat16, dev)
        Sl = S // world
        loc = [torch.cat([x[:, :, rank * Sl:(rank + 1) * Sl], x[:, :, S:]], dim=2).contiguous().requires_grad_(True)
               for x in (q, k, v)]
        s = sc.clone().requires_grad_(True)
        kw = dict(model=cfg["model"], text_valid=cfg["text_valid"], lowres_group_info=_group_info(cfg, dev),
                  window_size=cfg["window"], tile_size=cfg["tile"], latent_shape=cfg["latent"])

        def step():
            out = sp_soft_mixture_attention_autograd(*loc, T, s, **kw)
            out.float().sum().backward()
            for x in loc + [s]:
                x.grad = None

        dist.barrier()
        res[name] = _time(step, warmup, iters)
    ret[rank] = res
    dist.barrier()
    SP_STATE.cleanup()


def _single(warmup, iters):
    from vorta_amd.routed import geometry_for, soft_mixture_attention_autograd
    dev = torch.device("cuda:0")
    res = {}
    for name, cfg in SHAPES.items():
        q, k, v, sc, S, T = _inputs(cfg, torch.bfloat16, dev)
        L = [x.requires_grad_(True) for x in (q, k, v, sc)]
        geom = geometry_for(cfg["latent"], cfg["tile"], cfg["window"], cfg["group"], cfg["rate"], dev)

        def step():
            out = soft_mixture_attention_autograd(*L, geom, model=cfg["model"], text_len=T, text_valid=cfg["text_valid"])
            out.float().sum().backward()
            for x in L:
                x.grad = None

        res[name] = _time(step, warmup, iters)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    args = ap.parse_args()
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    with socket.socket() as sck:
        sck.bind(("127.0.0.1", 0))
        port = sck.getsockname()[1]
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, ret, args.warmup, args.iters)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=600)
        if any(p.is_alive() or p.exitcode != 0 for p in procs):
            for p in procs:
                p.kill()
            sys.exit("a rank failed or ran out of time")
        sp = {name: max(ret[r][name] for r in range(2)) for name in SHAPES}
    one = _single(args.warmup, args.iters)
    rep = {"what": "one soft-mixture layer, forward + backward, bf16, mean ms over the timed iterations",
           "world": 2, "transport": "gloo, staged through the host; both ranks share ONE GPU",
           "caveat": "a record, not a gate: ranks sharing a GPU say nothing about a wire; this exchange has not been "
                     "measured between GPUs",
           "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "iters": args.iters,
           "shapes": {name: {"heads": cfg["heads"], "tokens": cfg["latent"][0] * cfg["latent"][1] * cfg["latent"][2],
                             "text": cfg["text"], "sp_ms_slowest_rank": round(sp[name], 3),
                             "single_gpu_ms": round(one[name], 3)} for name, cfg in SHAPES.items()}}
    line = json.dumps(rep)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rep, indent=1) + "\n")


if __name__ == "__main__":
    main()
