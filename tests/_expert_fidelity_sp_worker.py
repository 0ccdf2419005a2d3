"""Worker of tests/test_hip_expert_fidelity_sp.py: what the gloo ranks that share the one GPU run (spawned processes import
this module).  Cases and geometry: tests/_sp_soft_mixture.py; rank set-up: tests/test_hip_sp_soft_mixture.py."""
import torch

import _sp_soft_mixture as C

FIELDS = ("sq_ref", "max_ref", "sq_err", "max_err")


def _np(fid):
    return {n: getattr(fid, n).detach().cpu().numpy() for n in FIELDS}


def fidelity_worker(rank, world, port, ret, model, H, dtype_name):
    """the forward-only and the differentiable operator with `fidelity=[...]` on this rank's shard; the ranks' statistics
    gathered over the group; rank 0 adds the single-process operator's on the same tensors"""
    import test_hip_sp_soft_mixture as M
    dist, SP = M._setup(rank, world, port)
    from vorta_amd import ops
    from vorta_amd.attention._sp import (gather_fidelity, mixture_head_range, sp_soft_mixture_attention,
                                         sp_soft_mixture_attention_autograd)
    dtype = M.DTYPES[dtype_name]
    T, te = C.text_of(model)
    q, k, v, sc, _ = C.operator_case(model, H, dtype)
    kw = dict(C.geometry_kw(), model=model, text_valid=te)
    loc = [C.shard(x, rank, world) for x in (q, k, v)]
    plain = sp_soft_mixture_attention(*loc, T, sc, **kw).clone()
    filed = []
    out = sp_soft_mixture_attention(*loc, T, sc, fidelity=filed, **kw).clone()
    leaves = [x.clone().requires_grad_(True) for x in loc] + [sc.clone().requires_grad_(True)]
    filed_grad = []
    out_grad = sp_soft_mixture_attention_autograd(*leaves[:3], T, leaves[3], fidelity=filed_grad, **kw)
    out_grad.float().sum().backward()
    torch.cuda.synchronize()
    h0, h1 = mixture_head_range(H)
    mine = dict(
        heads=(h0, h1), n_filed=(len(filed), len(filed_grad)),
        is_fidelity=isinstance(filed[0], ops.ExpertFidelity),
        local_shapes=[tuple(getattr(filed[0], n).shape) for n in FIELDS],
        n=filed[0].n,
        out_same=torch.equal(out, plain) and torch.equal(out_grad.detach(), plain),
        grad_form_same=all(torch.equal(getattr(filed[0], n), getattr(filed_grad[0], n)) for n in FIELDS),
        grads_finite=all(x.grad is not None and bool(torch.isfinite(x.grad).all()) for x in leaves))
    gathered = gather_fidelity(filed[0], H)  # a collective: every rank
    per_rank = M._gather(dist, mine)
    if rank == 0:
        from vorta_amd.routed import geometry_for, soft_mixture_attention
        geom = geometry_for(C.LATENT, C.TILE, C.WINDOW, C.GROUP, C.RATE, C.dev())
        one = []
        soft_mixture_attention(q, k, v, sc, geom, model=model, text_len=T, text_valid=te, fidelity=one)
        torch.cuda.synchronize()
        ret["res"] = dict(per_rank=per_rank, got=_np(gathered), one=_np(one[0]), n=(gathered.n, one[0].n),
                          rows=(C.S // world, C.S + T))
    dist.barrier()
    SP.cleanup()
