"""Child process of tests/test_hip_sp_soft_mixture.py: the differentiable soft mixture on ONE rank with a REAL RCCL process
group (backend "nccl") and VORTA_SP_FORCE_COLLECTIVES=1, as tests/_rccl_single_rank.py does for the inference exchange.

The gloo rehearsals take the host-staged branch of the exchange; this run takes the direct one -- `all_to_all_single(...,
async_op=True)` for q, k, v, the output, d_out and dq, dk, dv (three together), the text all-gather -- on a world of one,
where every collective is a copy RCCL performs on its own stream.  A missing wait shows as a mismatch against the single-GPU
operator.  Prints one JSON line: per tensor (error of this run, error of the single-GPU operator), both against float64 --
the oracle for the forward, autograd of the restated launches for the backward.  It cannot prove anything about peers."""
import datetime
import json
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sp_soft_mixture as C  # noqa: E402


def main():
    from vorta_amd.routed import geometry_for, soft_mixture_attention_autograd, sp_soft_mixture_attention_autograd
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=C.dev(), timeout=datetime.timedelta(seconds=60))
    model, H, dtype = "hunyuan", 4, torch.bfloat16
    T, te = C.text_of(model)
    q, k, v, sc, cot = C.operator_case(model, H, dtype)
    calls = {}

    def counted(name):
        fn = getattr(dist, name)

        def wrapper(*a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **kw)
        setattr(dist, name, wrapper)
    for name in ("all_to_all_single", "all_gather", "all_reduce", "batch_isend_irecv"):
        counted(name)

    def run(op):
        L = [x.clone().requires_grad_(True) for x in (q, k, v, sc)]
        out = op(*L)
        (out * cot).sum().backward()
        torch.cuda.synchronize()
        return out.detach()[0].transpose(0, 1), [x.grad for x in L]  # (H, N, D)

    with C.RecordSp() as rec:
        out_sp, g_sp = run(lambda a, b, c, s: sp_soft_mixture_attention_autograd(a, b, c, T, s, **C.geometry_kw(), model=model,
                                                                                  text_valid=te))
    counts = dict(calls)
    geom = geometry_for(C.LATENT, C.TILE, C.WINDOW, C.GROUP, C.RATE, C.dev())
    out_1, g_1 = run(lambda a, b, c, s: soft_mixture_attention_autograd(a, b, c, s, geom, model=model, text_len=T,
                                                                        text_valid=te).transpose(1, 2))
    ref = torch.as_tensor(C.oracle_forward(model, q, k, v, sc)[0]).to(C.dev())
    g64, _ = C.reference_grads(q, k, v, sc, cot, C.globalize(rec.calls[0], 0), torch.float64)
    pairs = {"out": (C.rel_err(out_sp, ref), C.rel_err(out_1, ref))}
    for name, a, b, r in zip(("dq", "dk", "dv", "dscores"), g_sp, g_1, g64):
        pairs[name] = (C.rel_err(a.reshape(r.shape), r), C.rel_err(b.reshape(r.shape), r))
    backend = dist.get_backend()
    dist.barrier()
    dist.destroy_process_group()
    print(json.dumps({"backend": backend, "collective_calls": counts, "pairs": pairs,
                      "bits_equal": bool(torch.equal(out_sp, out_1))}), flush=True)


if __name__ == "__main__":
    main()
