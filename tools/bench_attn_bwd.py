"""Forward and backward time of the gather attention at model size (recorded, not gated; bench.py is the project's yardstick
and is not involved).

    python tools/bench_attn_bwd.py --case dense   --config hunyuan-129f     one dense head
    python tools/bench_attn_bwd.py --case mixture --config wan1.3b-49f      the full soft-mixture layer, every head
    python tools/bench_attn_bwd.py --all --out profiles/attn_bwd_timing.json
    python tools/bench_attn_bwd.py --all --algorithm both --out profiles/attn_bwd_key_major_timing.json
    python tools/bench_attn_bwd.py --all --algorithm all --out profiles/attn_bwd_deterministic_timing.json

`--all` runs the four (case, config) steps as child processes, each under its own `timeout -k 10`, in a chain that stops at
the first step that fails (the shell form: `timeout -k 10 600 python tools/bench_attn_bwd.py --case dense --config
hunyuan-129f && timeout -k 10 600 ...`), and collects their JSON lines.  The yardstick of the backward figure is the forward of
the SAME launches in the same process; FLOPs count the five products of the backward plus the recomputed scores (6 / 2 of
the forward's 4 S_q S_kv D per head).

`--algorithm query_major` (the default) times vorta_attn_bwd, `key_major` the statistics pass + vorta_attn_bwd_kmajor, `both`
the two side by side in one process, with the bytes each adds with float atomics and bytes / time against the chip-wide rate
of such adds (ATOMIC_RATE): a kernel near it is bound by its atomics whatever its loop does.  `deterministic` times the
statistics pass + vorta_attn_bwd_dq + vorta_attn_bwd_dkv (no atomic bytes) and reports the three passes on their own
(stats_ms, dq_ms, dkv_ms) with the kernel launches the dK / dV pass issues per recorded launch (one per key list); `all` the
three algorithms and the forward in one process, alternating over ROUNDS rounds (bwd_ms: the mean; bwd_ms_rounds: each)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ATOMIC_RATE = 1.3e12  # bytes / s of float atomic adds, chip-wide (MI355X; measured at 1.26-1.36e12 for every placement)
ROUNDS = 2  # of `--algorithm all`: forward and the three algorithms take turns, so that a drift of the clock shows in all of them
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


def atomic_bytes(c, H):
    """(query-major, key-major, deterministic) bytes one recorded launch adds with float atomics.  Query-major: every 128-row query block
    adds the dK and dV rows of all its keys.  Key-major: every live query row is added once per 256-key block (dQ), every
    key row of a group with a live query once (dK, dV)."""
    heads = c.get("n_heads") or (c["head_list"].numel() if c.get("head_list") is not None else H)
    n_q, n_kv = c["n_q"], c["n_kv"]
    q_valid = n_q if c.get("q_valid") is None else c["q_valid"]
    if c.get("q_block_table") is not None:
        rows = c["q_block_table"].cpu().tolist()
    else:
        glen = c.get("q_group_len", 0) or n_q
        rows = [(g, g * glen, min((g + 1) * glen, n_q)) for g in range(-(-n_q // glen))]
    live = [(g, a, min(b, q_valid)) for g, a, b in rows if min(b, q_valid) > a]
    row_bytes = 128 * 4
    qm = sum(-(-(b - a) // 128) for _, a, b in rows if b > a) * n_kv * row_bytes * 2
    km = sum(b - a for _, a, b in live) * -(-n_kv // 256) * row_bytes + len({g for g, _, _ in live}) * n_kv * row_bytes * 2
    return heads * qm, heads * km, 0


def key_lists(c):
    """kernel launches vorta_attn_bwd_dkv issues for one recorded launch: one per key list"""
    if c.get("q_block_table") is not None:
        return c["n_key_lists"]
    return -(-c["n_q"] // (c.get("q_group_len", 0) or c["n_q"]))


def run_one(case, config, warmup, steps, algorithm="query_major"):
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
    bwd_by = lambda alg: (lambda: routed._replay_backward(launches, g[0], acc[0], acc[1], acc[2], weight_of,  # noqa: E731
                                                          algorithm=alg))

    def each_launch(fn):
        for i, c in enumerate(launches):
            c = dict(c)
            x = [c.pop(n) for n in ("q", "k", "v", "out")]
            fn(i, x, dict(c, do_scale=None if weight_of is None else weight_of(c, x[3])))

    kept = {}  # launch -> its statistics (the dQ and dK / dV passes alone read the ones a first statistics pass left)
    stats_only = lambda: each_launch(lambda i, x, kw: kept.__setitem__(i, ops.attn_bwd_stats(*x, g[0], **kw)))  # noqa: E731
    dq_only = lambda: each_launch(lambda i, x, kw: ops.attn_bwd_dq(*x, g[0], acc[0], kept[i], **kw))  # noqa: E731
    dkv_only = lambda: each_launch(lambda i, x, kw: ops.attn_bwd_dkv(*x, g[0], acc[1], acc[2], kept[i], **kw))  # noqa: E731

    def parts(alg):
        """the passes of an algorithm on their own"""
        if alg == "query_major":
            return {}
        out = dict(stats_ms=round(_time(stats_only, warmup, steps), 3))
        if alg == "deterministic":
            out.update(dq_ms=round(_time(dq_only, warmup, steps), 3), dkv_ms=round(_time(dkv_only, warmup, steps), 3),
                       dkv_kernel_launches=[key_lists(c) for c in launches])
        return out

    fwd_ms = _time(fwd, warmup, steps)
    fwd_flops = sum(c.get("flops", 0.0) for c in launches)
    res = dict(case=case, config=config, dtype=cfg["dtype"], heads=H, tokens=S + T, launches=len(launches),
               warmup=warmup, steps=steps, fwd_ms=round(fwd_ms, 3))
    per = lambda ms: dict(bwd_ms=round(ms, 3), bwd_over_fwd=round(ms / fwd_ms, 3),  # noqa: E731
                          bwd_tflops=round(3.0 * fwd_flops / ms / 1e9, 1))
    if algorithm not in ("both", "all"):
        res.update(per(_time(bwd_by(algorithm), warmup, steps)), fwd_tflops=round(fwd_flops / fwd_ms / 1e9, 1))
        if algorithm != "query_major":
            res.update(algorithm=algorithm, **parts(algorithm))
    else:
        algs = routed.ATTENTION_BACKWARDS if algorithm == "all" else ("query_major", "key_major")
        nbytes = dict(zip(routed.ATTENTION_BACKWARDS, map(sum, zip(*(atomic_bytes(c, H) for c in launches)))))
        rounds = {alg: [] for alg in algs}
        fwd_rounds = [fwd_ms]
        for r in range(ROUNDS if algorithm == "all" else 1):
            if r:
                fwd_rounds.append(_time(fwd, warmup, steps))
            for alg in algs:
                rounds[alg].append(_time(bwd_by(alg), warmup, steps))
        if algorithm == "all":
            fwd_ms = sum(fwd_rounds) / len(fwd_rounds)
            res.update(fwd_ms=round(fwd_ms, 3), fwd_ms_rounds=[round(x, 3) for x in fwd_rounds])
        res["fwd_tflops"] = round(fwd_flops / fwd_ms / 1e9, 1)
        for alg in algs:
            ms = sum(rounds[alg]) / len(rounds[alg])
            res[alg] = dict(per(ms), atomic_bytes=nbytes[alg], atomic_floor_ms=round(nbytes[alg] / ATOMIC_RATE * 1e3, 3),
                            atomic_tb_per_s=round(nbytes[alg] / ms / 1e9, 3),
                            of_atomic_rate=round(nbytes[alg] / (ms * 1e-3) / ATOMIC_RATE, 3))
            if algorithm == "all":
                res[alg]["bwd_ms_rounds"] = [round(x, 3) for x in rounds[alg]]
            res[alg].update(parts(alg))
        res["key_major_speedup"] = round(res["query_major"]["bwd_ms"] / res["key_major"]["bwd_ms"], 3)
        if algorithm == "all":
            for alg in ("query_major", "key_major"):
                res["deterministic_over_" + alg] = round(res["deterministic"]["bwd_ms"] / res[alg]["bwd_ms"], 3)
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["dense", "mixture"])
    ap.add_argument("--config", default="hunyuan-129f")
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--algorithm", choices=["query_major", "key_major", "deterministic", "both", "all"], default="query_major")
    ap.add_argument("--out")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=280)
    a = ap.parse_args()
    if not a.all:
        print(json.dumps(run_one(a.case, a.config, a.warmup, a.steps, a.algorithm)), flush=True)
        return 0
    results = []
    for case, config in STEPS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--case", case,
               "--config", config, "--warmup", str(a.warmup), "--steps", str(a.steps), "--algorithm", a.algorithm]
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
                                "and launch for the forward and 3 x that (5 products + the recomputed scores) for the backward"
                                + ("; atomic_bytes = bytes added with float atomics, atomic_floor_ms = those bytes at the "
                                   "chip-wide rate of 1.3 TB/s, of_atomic_rate = bytes / time against that rate; key_major's "
                                   "bwd_ms includes its statistics pass (stats_ms, timed alone)" if a.algorithm in ("both", "all") else "")
                                + ("; deterministic's bwd_ms = statistics + dQ + dK / dV passes (stats_ms, dq_ms, dkv_ms: each timed "
                                   "alone), dkv_kernel_launches = kernel launches of the dK / dV pass per recorded launch (one per key "
                                   "list); forward and algorithms alternate over two rounds (bwd_ms: the mean)"
                                   if a.algorithm == "all" else ""),
                           results=results), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
