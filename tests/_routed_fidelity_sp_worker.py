"""Worker of tests/test_hip_routed_fidelity_sp.py: `sp_attention(..., fidelity=[...])` on this rank's shard, the ranks' records
joined by `gather_routed_fidelity`, beside the single-process `routed_attention(..., fidelity=[...])` on the same tensors, table
and routes.  Imported by the gloo ranks that share the one GPU (`routed_worker`; rank set-up: tests/test_hip_sp_soft_mixture.py),
and run as a script for ONE rank with a real RCCL group (backend "nccl", VORTA_SP_FORCE_COLLECTIVES=1: the direct branch of the
exchange), which prints one JSON line.  Cases and geometry: tests/_sp_soft_mixture.py (latent (12, 6, 8), S = 576)."""
import datetime
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sp_soft_mixture as C  # noqa: E402

FIELDS = ("sq_ref", "max_ref", "range_ref", "sq_err", "max_err")
N_ROWS = 64
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _np(fid):
    d = {n: getattr(fid, n).detach().cpu().numpy() for n in FIELDS}
    d["expert"] = fid.expert.cpu().tolist()
    return d


def measure(rank, world, model, H, dtype, experts, placement, heads):
    """(this rank's facts, the gathered record, the placement's split heads): the sequence-parallel call twice, without and
    with a sink"""
    import vorta_amd.attention._sp as sp
    sp.SP_PLACEMENT = placement
    seen, stock = [], sp.place_heads

    def spy(*a, **kw):
        res = stock(*a, **kw)
        seen.append(res)
        return res

    sp.place_heads = spy
    T, te = C.text_of(model)
    q, k, v, sc, _ = C.operator_case(model, H, dtype)
    kw = dict(C.geometry_kw(), model=model, text_valid=te, experts_host=list(experts))
    loc = [C.shard(x, rank, world) for x in (q, k, v)]
    plain = sp.sp_attention(*loc, T, sc, 0.0, **kw).clone()
    filed = []
    out = sp.sp_attention(*loc, T, sc, 0.0, fidelity=filed, fidelity_rows=N_ROWS, fidelity_heads=heads, **kw).clone()
    torch.cuda.synchronize()
    _, order, counts, parts = seen[-1]
    split = sorted({order[i] for i, p in enumerate(parts or ()) if p is not None})
    rec = filed[0]
    mine = dict(n_filed=len(filed), out_same=bool(torch.equal(out, plain)), shape=tuple(rec.sq_err.shape), n=rec.n,
                local_heads=(rec.expert >= 0).nonzero().flatten().tolist(), counts=list(counts), taken=seen[-1][0],
                rows=rec.rows.cpu().tolist())
    gathered = sp.gather_routed_fidelity(rec)  # a collective: every rank
    return mine, gathered, split, (q, k, v, T, te)


def single_process(q, k, v, T, te, model, experts, heads):
    from vorta_amd.routed import HeadRouting, geometry_for, routed_attention
    geom = geometry_for(C.LATENT, C.TILE, C.WINDOW, C.GROUP, C.RATE, C.dev())
    one = []
    routed_attention(q, k, v, HeadRouting.from_expert_ids(list(experts), C.dev()), geom, model=model, text_len=T, text_valid=te,
                     fp8="native", fidelity=one, fidelity_rows=N_ROWS, fidelity_heads=heads)
    torch.cuda.synchronize()
    return one[0]


def routed_worker(rank, world, port, ret, model, H, dtype_name, experts, placement, heads):
    import test_hip_sp_soft_mixture as M
    dist, SP = M._setup(rank, world, port)
    mine, gathered, split, (q, k, v, T, te) = measure(rank, world, model, H, DTYPES[dtype_name], experts, placement, heads)
    per_rank = M._gather(dist, mine)
    if rank == 0:
        one = single_process(q, k, v, T, te, model, experts, heads)
        ret["res"] = dict(per_rank=per_rank, got=_np(gathered), one=_np(one), n=(gathered.n, one.n), split=split,
                          rows=(gathered.rows.cpu().tolist(), one.rows.cpu().tolist()))
    dist.barrier()
    SP.cleanup()


def main():
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=C.dev(), timeout=datetime.timedelta(seconds=60))
    calls = {}

    def counted(name):
        fn = getattr(dist, name)

        def wrapper(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **kw)
        setattr(dist, name, wrapper)
    for name in ("all_to_all_single", "all_gather", "all_reduce"):
        counted(name)
    model, H, experts, heads = "hunyuan", 4, [0, 1, 2, 1], "all"
    mine, gathered, split, (q, k, v, T, te) = measure(0, 1, model, H, torch.bfloat16, experts, "auto", heads)
    one = single_process(q, k, v, T, te, model, experts, heads)
    backend = dist.get_backend()
    dist.barrier()
    dist.destroy_process_group()
    as_lists = lambda d: {n: (x if isinstance(x, list) else x.astype("float64").tolist()) for n, x in d.items()}  # noqa: E731
    print(json.dumps({"backend": backend, "collective_calls": calls, "mine": mine, "got": as_lists(_np(gathered)),
                      "one": as_lists(_np(one)), "split": split}), flush=True)


if __name__ == "__main__":
    main()
