#!/usr/bin/env python3
"""One layer of the soft mixture, forward + backward, under sequence parallelism.  Two legs:

    python tools/bench_sp_soft_mixture.py --out profiles/sp_soft_mixture_timing.json
    python tools/bench_sp_soft_mixture.py --leg rank-of-eight --algorithm all --out profiles/sp_soft_mixture_backward_timing.json

`--leg rehearsal` (default): two gloo ranks SHARING one GPU, beside the single-GPU operator on the whole sequence.  A record,
not a gate.  Ranks that share a GPU say nothing about a wire: the exchange is staged through the host (gloo cannot move device
memory) and the two ranks' kernels compete for the same CUs, so `sp_ms` is NOT what two GPUs would take.  Nobody has measured
this exchange between GPUs.  What the figure does show: the whole path runs at these sizes, and what the host-staged rehearsal
costs.  `--algorithm` picks the attention backward (`all`: one after the other in the same ranks).

`--leg rank-of-eight`: ONE process, no process group, no exchange -- what a rank computes between its exchanges.
`_RecvSoftMixture` forward and backward on random receive buffers in the layout of rank 0 of 8 at Hunyuan-129f (3 local heads
of 24, 118 800 video tokens + 256 text rows, row tables composed with the layout's row map, head stride S/8 rows).  The
algorithms take turns inside every round, so that a drift of the clock shows in all of them; device-event times, a warm-up per
algorithm, every round kept.  The yardstick is `query_major` in the same process."""
import argparse
import json
import os
import socket
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALGORITHMS = ("query_major", "key_major", "deterministic")

SHAPES = {
    # the shape of tests/test_hip_sp_soft_mixture.py
    "test": dict(model="hunyuan", latent=(12, 6, 8), tile=(2, 3, 4), window=(3, 3, 3), group=(2, 3, 2), rate=0.5, heads=4,
                 text=8, text_valid=5),
    # bench.py CONFIGS["wan1.3b-49f"]
    "wan1.3b-49f": dict(model="wan", latent=(13, 20, 32), tile=(13, 10, 8), window=(3, 3, 3), group=(1, 2, 2), rate=0.5,
                        heads=12, text=0, text_valid=0),
}
# bench.py CONFIGS["hunyuan-129f"] on 8 ranks: the layer the soft mixture is trained at
RANK_OF_EIGHT = dict(model="hunyuan", latent=(33, 45, 80), tile=(11, 9, 8), window=(3, 3, 3), group=(3, 3, 2), rate=0.5,
                     heads=24, text=256, text_valid=96, world=8, rank=0)


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


def _worker(rank, world, port, ret, warmup, iters, algorithms):
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
        res[name] = {}
        for alg in algorithms:
            def step():
                out = sp_soft_mixture_attention_autograd(*loc, T, s, backward=alg, **kw)
                out.float().sum().backward()
                for x in loc + [s]:
                    x.grad = None

            dist.barrier()
            res[name][alg] = _time(step, warmup, iters)
    ret[rank] = res
    dist.barrier()
    SP_STATE.cleanup()


def _single(warmup, iters, algorithms):
    from vorta_amd.routed import geometry_for, soft_mixture_attention_autograd
    dev = torch.device("cuda:0")
    res = {}
    for name, cfg in SHAPES.items():
        q, k, v, sc, S, T = _inputs(cfg, torch.bfloat16, dev)
        L = [x.requires_grad_(True) for x in (q, k, v, sc)]
        geom = geometry_for(cfg["latent"], cfg["tile"], cfg["window"], cfg["group"], cfg["rate"], dev)
        res[name] = {}
        for alg in algorithms:
            def step():
                out = soft_mixture_attention_autograd(*L, geom, model=cfg["model"], text_len=T, text_valid=cfg["text_valid"],
                                                      backward=alg)
                out.float().sum().backward()
                for x in L:
                    x.grad = None

            res[name][alg] = _time(step, warmup, iters)
    return res


def rehearsal(args, algorithms):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    with socket.socket() as sck:
        sck.bind(("127.0.0.1", 0))
        port = sck.getsockname()[1]
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, ret, args.warmup, args.iters, algorithms)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=600)
        if any(p.is_alive() or p.exitcode != 0 for p in procs):
            for p in procs:
                p.kill()
            sys.exit("a rank failed or ran out of time")
        sp = {name: {alg: max(ret[r][name][alg] for r in range(2)) for alg in algorithms} for name in SHAPES}
    one = _single(args.warmup, args.iters, algorithms)
    shapes = {}
    for name, cfg in SHAPES.items():
        shapes[name] = {"heads": cfg["heads"], "tokens": cfg["latent"][0] * cfg["latent"][1] * cfg["latent"][2], "text": cfg["text"]}
        if len(algorithms) == 1:
            shapes[name].update(sp_ms_slowest_rank=round(sp[name][algorithms[0]], 3), single_gpu_ms=round(one[name][algorithms[0]], 3))
        else:
            shapes[name]["by_algorithm"] = {alg: {"sp_ms_slowest_rank": round(sp[name][alg], 3),
                                                  "single_gpu_ms": round(one[name][alg], 3)} for alg in algorithms}
    return {"what": "one soft-mixture layer, forward + backward, bf16, mean ms over the timed iterations",
            "world": 2, "transport": "gloo, staged through the host; both ranks share ONE GPU",
            "caveat": "a record, not a gate: ranks sharing a GPU say nothing about a wire; this exchange has not been "
                      "measured between GPUs",
            "attention_backward": list(algorithms),
            "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "iters": args.iters, "shapes": shapes}


def rank_of_eight(args, algorithms):
    from vorta_amd.attention._sp import _RecvSoftMixture
    from vorta_amd.routed import geometry_for
    from vorta_amd.ulysses.engine import UlyssesLayout
    cfg, dev, dtype = RANK_OF_EIGHT, torch.device("cuda:0"), torch.bfloat16
    torch.cuda.set_device(0)
    S = cfg["latent"][0] * cfg["latent"][1] * cfg["latent"][2]
    lay = UlyssesLayout(H=cfg["heads"], S=S, T=cfg["text"], D=128, P=cfg["world"], rank=cfg["rank"], device=dev, dtype=dtype)
    geom = geometry_for(cfg["latent"], cfg["tile"], cfg["window"], cfg["group"], cfg["rate"], dev, row_map=lay.row_map)
    g = torch.Generator(device=dev).manual_seed(1)
    rand = lambda: torch.randn((lay.rows_total, lay.D), generator=g, device=dev).to(dtype)  # noqa: E731
    qb, kb, vb = (rand().requires_grad_(True) for _ in range(3))
    d_ob = rand()
    sc = torch.softmax(torch.randn((1, lay.Hl, 3), generator=g, device=dev), dim=-1).to(dtype).requires_grad_(True)
    leaves = [qb, kb, vb, sc]

    def timed(alg, n):
        """n forward + backward passes under `alg`: (forward ms, backward ms) per pass, from device events"""
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)]
        for e in ev:
            e[0].record()
            ob = _RecvSoftMixture.apply(qb, kb, vb, sc, lay, geom, cfg["model"], cfg["text"], cfg["text_valid"], None, alg)
            e[1].record()
            ob.backward(d_ob)
            e[2].record()
            for x in leaves:
                x.grad = None
        torch.cuda.synchronize()
        return [e[0].elapsed_time(e[1]) for e in ev], [e[1].elapsed_time(e[2]) for e in ev]

    for alg in algorithms:
        timed(alg, args.warmup)
    fwd = {alg: [] for alg in algorithms}
    bwd = {alg: [] for alg in algorithms}
    for _ in range(args.rounds):
        for alg in algorithms:  # the algorithms take turns inside a round
            f, b = timed(alg, args.iters)
            fwd[alg].append(sum(f) / len(f))
            bwd[alg].append(sum(b) / len(b))
    mean = lambda xs: sum(xs) / len(xs)  # noqa: E731
    res = {}
    for alg in algorithms:
        res[alg] = {"fwd_ms": round(mean(fwd[alg]), 3), "bwd_ms": round(mean(bwd[alg]), 3),
                    "fwd_ms_rounds": [round(x, 3) for x in fwd[alg]], "bwd_ms_rounds": [round(x, 3) for x in bwd[alg]]}
    if "query_major" in res:
        for alg in algorithms:
            res[alg]["bwd_over_query_major"] = round(res[alg]["bwd_ms"] / res["query_major"]["bwd_ms"], 4)
            res[alg]["bwd_over_query_major_rounds"] = [round(x / y, 4) for x, y in zip(bwd[alg], bwd["query_major"])]
    return {"what": "one rank's share of one soft-mixture layer between its exchanges: _RecvSoftMixture forward and backward "
                    "(three experts, mix, mix backward, replayed attention backward, cast) on random receive buffers, bf16; ms "
                    "from device events, the mean over `iters` passes per round, every round kept",
            "layout": {"config": "hunyuan-129f", "heads": cfg["heads"], "world": cfg["world"], "rank": cfg["rank"],
                       "local_heads": lay.Hl, "video_tokens": S, "text_rows": cfg["text"], "text_valid": cfg["text_valid"],
                       "rows_per_shard": lay.Sl, "rows_total": lay.rows_total},
            "caveat": "one process, no process group, no exchange: the compute of a rank, not a training step; the yardstick is "
                      "query_major in the same process",
            "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "iters": args.iters, "rounds": args.rounds,
            "order": "the algorithms take turns inside every round", "algorithms": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", choices=("rehearsal", "rank-of-eight"), default="rehearsal")
    ap.add_argument("--algorithm", choices=ALGORITHMS + ("all",), default="query_major",
                    help="the attention backward (all: every one, taking turns)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="rank-of-eight: rounds in which the algorithms take turns")
    args = ap.parse_args()
    algorithms = ALGORITHMS if args.algorithm == "all" else (args.algorithm,)
    rep = rehearsal(args, algorithms) if args.leg == "rehearsal" else rank_of_eight(args, algorithms)
    line = json.dumps(rep)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(rep, indent=1) + "\n")


if __name__ == "__main__":
    main()
