"""GPU: the soft mixture under sequence parallelism on a PARTIAL geometry -- two gloo ranks that share the one GPU (the spawn
pattern of tests/test_hip_sp_soft_mixture.py).  The partial tables compose with the Ulysses row map as the dividing ones do;
the token shard needs P to divide S (378 = 2 x 189 here).  Two paths: the training operator
(`sp_soft_mixture_attention[_autograd]`) and routed inference (`sp_attention`, behind the Eval processors).  Forward: every row of every head against the float64 restatement
(tests/_partial_geometry_restate.py) at tests/_util.check's tolerances.  Backward: the assembled gradients (video shards
concatenated, text rows and score gradients summed over the ranks) under the rule of tests/test_hip_attention_bwd.py."""
import numpy as np
import pytest
import torch

import _partial_geometry_restate as R
from test_hip_sp_soft_mixture import _gather, _run, _setup

pytestmark = pytest.mark.gpu

LATENT, TILE, WINDOW, GROUP = (7, 9, 6), (2, 2, 4), (3, 3, 3), (2, 2, 2)
S = 7 * 9 * 6
H = 4


def _worker(rank, world, port, ret, model):
    from vorta_amd import _partial
    _partial.set_partial_geometry(True)
    dist, SP = _setup(rank, world, port)
    from _sp_soft_mixture import shard
    from _util import check, dev
    from test_hip_attention_bwd import _bound
    from test_hip_partial_geometry import _kernel_choice, _recorded
    from vorta_amd.attention import get_group_info
    from vorta_amd.routed import geometry_for, sp_soft_mixture_attention, sp_soft_mixture_attention_autograd
    dtype = torch.bfloat16
    T, te = (64, 40) if model == "hunyuan" else (0, 0)
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn((1, H, S + T, 128), generator=g).to(dtype).to(dev()) for _ in range(3))
    sc = torch.softmax(torch.randn((1, H, 3), generator=g), dim=-1).to(dtype).to(dev())
    cot = torch.randn((1, S + T, H, 128), generator=g).to(dtype).to(dev())
    kw = dict(lowres_group_info=get_group_info(LATENT, GROUP, 0.5, dev()), window_size=WINDOW, tile_size=TILE,
              latent_shape=LATENT, model=model, text_valid=te)
    loc = [shard(x, rank, world, S).requires_grad_(True) for x in (q, k, v)]
    s = sc.clone().requires_grad_(True)
    out0 = sp_soft_mixture_attention(*[x.detach() for x in loc], T, sc, **kw)
    out = sp_soft_mixture_attention_autograd(*loc, T, s, backward="deterministic", **kw)
    (out * shard(cot, rank, world, S, dim=1)).sum().backward()
    torch.cuda.synchronize()
    n = lambda t: t.detach().float().cpu()  # noqa: E731
    got = _gather(dist, dict(out=n(out[0]), grads=[n(x.grad[0]) for x in loc], dsc=n(s.grad), same=torch.equal(out, out0)))
    if rank == 0:
        Sl = S // world
        t = lambda a: a.to(dev())  # noqa: E731
        full = torch.cat([t(p["out"])[:Sl] for p in got] + [t(got[0]["out"])[Sl:]], dim=0).transpose(0, 1)  # (H, S+T, D)
        assert all(p["same"] for p in got)  # the grad form gives the bits of the no_grad form
        assert all(torch.equal(p["out"][Sl:], got[0]["out"][Sl:]) for p in got)  # every rank holds the same text rows
        geom = geometry_for(LATENT, TILE, WINDOW, GROUP, 0.5, dev())
        assert geom.is_partial
        cs = R.Coreset(LATENT, GROUP)
        _, launches = _recorded(q, k, v, geom, model)  # the single-process launches: the kernel's own margin choice
        specs = R.expert_specs(LATENT, TILE, WINDOW, cs, *_kernel_choice(launches, cs, te), T, te)
        f64 = lambda x: x[0].double().cpu().numpy()  # noqa: E731
        ref = R.mixture(f64(q), f64(k), f64(v), sc[0].double().cpu().numpy(), specs)
        for h in range(H):
            check(full[h].to(dtype), ref[h], dtype)

        def reference(dt):
            leaves = [x[0].detach().to(dt).requires_grad_(True) for x in (q, k, v)]
            s_ = sc[0].detach().to(dt).requires_grad_(True)
            return torch.autograd.grad(R.mixture_torch(*leaves, s_, specs), leaves + [s_], cot[0].transpose(0, 1).to(dt))

        r64, r16 = reference(torch.float64), reference(dtype)
        for i, name in enumerate(("dq", "dk", "dv")):
            video = torch.cat([t(p["grads"][i])[:, :Sl] for p in got], dim=1).double()
            text = sum(t(p["grads"][i])[:, Sl:].double() for p in got)
            _bound(name, torch.cat([video, text], dim=1), r16[i], r64[i], f"sp {model}")
        _bound("dscores", sum(t(p["dsc"]).double() for p in got)[0], r16[3], r64[3], f"sp {model}")
        ret["ok"] = True
    dist.barrier()
    SP.cleanup()


@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_soft_mixture_on_a_partial_geometry_under_sequence_parallelism(model):
    assert _run(_worker, 2, (model,))["ok"]


def _eval_worker(rank, world, port, ret, model):
    """routed INFERENCE (`sp_attention`, the Eval processors' path): the placement cost, the exchange and the routed launches
    through the receive layout's row map"""
    from vorta_amd import _partial
    _partial.set_partial_geometry(True)
    dist, SP = _setup(rank, world, port)
    from _sp_soft_mixture import rel_err, shard
    from _util import check, dev
    from test_hip_partial_geometry import _kernel_choice, _recorded
    from vorta_amd.attention import get_group_info
    from vorta_amd.attention._sp import sp_attention
    from vorta_amd.routed import HeadRouting, geometry_for, routed_attention
    dtype = torch.bfloat16
    T, te = (64, 40) if model == "hunyuan" else (0, 0)
    experts = [0, 1, 2, 1]
    g = torch.Generator().manual_seed(4)
    q, k, v = (torch.randn((1, H, S + T, 128), generator=g).to(dtype).to(dev()) for _ in range(3))
    score = torch.zeros((1, H, 3), dtype=dtype, device=dev())  # (not read: the routes come with `experts_host`)
    out = sp_attention(*[shard(x, rank, world, S) for x in (q, k, v)], T, score, 0.3, model=model, text_valid=te,
                       lowres_group_info=get_group_info(LATENT, GROUP, 0.5, dev()), window_size=WINDOW, tile_size=TILE,
                       latent_shape=LATENT, experts_host=experts)
    torch.cuda.synchronize()
    got = _gather(dist, out[0].detach().float().cpu())
    if rank == 0:
        Sl = S // world
        full = torch.cat([p[:Sl] for p in got] + [got[0][Sl:]], dim=0).transpose(0, 1).to(dev())  # (H, S+T, D)
        assert all(torch.equal(p[Sl:], got[0][Sl:]) for p in got)
        geom = geometry_for(LATENT, TILE, WINDOW, GROUP, 0.5, dev())
        assert geom.is_partial
        one = routed_attention(q, k, v, HeadRouting.from_expert_ids(experts, dev()), geom, model=model, text_len=T,
                               text_valid=te, fp8=False)[0]
        cs = R.Coreset(LATENT, GROUP)
        _, launches = _recorded(q, k, v, geom, model)
        specs = R.expert_specs(LATENT, TILE, WINDOW, cs, *_kernel_choice(launches, cs, te), T, te)
        f64 = lambda x: x[0].double().cpu().numpy()  # noqa: E731
        refs = [R.attend(f64(q), f64(k), f64(v), *specs[e]) for e in range(3)]
        ref = torch.as_tensor(np.stack([refs[e][h] for h, e in enumerate(experts)])).to(dev())
        for h in range(H):
            check(full[h].to(dtype), ref[h].cpu().numpy(), dtype)
        e_sp, e_one = rel_err(full, ref), rel_err(one, ref)
        print(f"sp_attention {model}: rel error {e_sp:.3e}, one GPU {e_one:.3e}, bits equal {torch.equal(full.to(dtype), one)}")
        assert e_sp <= 2.0 * e_one  # the factor between two 16-bit evaluations of one formula (tests/test_hip_sp_soft_mixture.py)
        ret["ok"] = True
    dist.barrier()
    SP.cleanup()


@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_routed_inference_on_a_partial_geometry_under_sequence_parallelism(model):
    assert _run(_eval_worker, 2, (model,))["ok"]
