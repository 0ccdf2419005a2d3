"""Child process of tests/test_hip_sp_soft_mixture_backward.py: the differentiable soft mixture with backward="deterministic"
on ONE rank with a REAL RCCL process group (backend "nccl") and VORTA_SP_FORCE_COLLECTIVES=1, as
tests/_rccl_single_rank_soft_mixture.py does for the query-major backward.

The exchanges of d_out and of dq, dk, dv then run on RCCL's stream while the statistics, dQ and dK / dV passes run on the
current one: a missing wait shows as a mismatch.  Prints one JSON line: per gradient (error of this run, error of torch's
16-bit autograd on the restated launches), both against float64 autograd of the same restatement; the calls of the backward
entry points; and, as a figure, whether the bits equal the single-GPU operator's under the same algorithm."""
import datetime
import json
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sp_soft_mixture as C  # noqa: E402
from _sp_backward_workers import SpyBackwardOps  # noqa: E402


def main():
    from vorta_amd.routed import geometry_for, soft_mixture_attention_autograd, sp_soft_mixture_attention_autograd
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=C.dev(), timeout=datetime.timedelta(seconds=60))
    model, H, dtype = "hunyuan", 4, torch.bfloat16
    T, te = C.text_of(model)
    q, k, v, sc, cot = C.operator_case(model, H, dtype)

    def run(op):
        L = [x.clone().requires_grad_(True) for x in (q, k, v, sc)]
        out = op(*L)
        (out * cot).sum().backward()
        torch.cuda.synchronize()
        return [x.grad for x in L]

    with C.RecordSp() as rec, SpyBackwardOps() as spy:
        g_sp = run(lambda a, b, c, s: sp_soft_mixture_attention_autograd(a, b, c, T, s, **C.geometry_kw(), model=model,
                                                                         text_valid=te, backward="deterministic"))
    calls, n_launches = dict(spy.calls), len(rec.calls[0][0])
    geom = geometry_for(C.LATENT, C.TILE, C.WINDOW, C.GROUP, C.RATE, C.dev())
    g_1 = run(lambda a, b, c, s: soft_mixture_attention_autograd(a, b, c, s, geom, model=model, text_len=T, text_valid=te,
                                                                 backward="deterministic").transpose(1, 2))
    launches = C.globalize(rec.calls[0], 0)
    g64, _ = C.reference_grads(q, k, v, sc, cot, launches, torch.float64)
    g16, _ = C.reference_grads(q, k, v, sc, cot, launches, dtype)
    pairs, bits = {}, {}
    for name, a, b, r, y in zip(("dq", "dk", "dv", "dscores"), g_sp, g_1, g64, g16):
        pairs[name] = (C.rel_err(a.reshape(r.shape), r), C.rel_err(y, r))
        bits[name] = bool(torch.equal(a, b))
    backend = dist.get_backend()
    dist.barrier()
    dist.destroy_process_group()
    print(json.dumps({"backend": backend, "calls": calls, "n_launches": n_launches, "pairs": pairs,
                      "bits_equal_single_gpu": bits}), flush=True)


if __name__ == "__main__":
    main()
