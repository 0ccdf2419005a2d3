"""GPU: the backward of the gather attention (vorta_attn_bwd) and of the soft mixture, against torch autograd in float64 on a
plain restatement (tests/_attn_restate.py) fed the same 16-bit-rounded inputs -- never the code under test.

Tolerance (measured, not guessed): the yardstick is torch's own 16-bit autograd (matmul / softmax in the launch's dtype) on
the same restatement.  Per case and gradient, e_torch = rel_fro(torch16, f64), e_hip = rel_fro(kernel, f64) and
e_hip <= 2 e_torch: the kernel rounds P and dS to 16 bits before their MFMAs where torch rounds after each operator -- the
same number of roundings in other places, so the errors are of one size and a factor of two separates "same size" from
"wrong".  A gradient whose float64 norm is exactly zero must be exactly zero."""
import os

import numpy as np
import pytest
import torch

import _random_launch as RL
from _attn_restate import named_rows, restate
from _util import dev

pytestmark = pytest.mark.gpu

LATENT, TILE, WINDOW, GROUP = (8, 6, 8), (2, 3, 4), (3, 3, 3), (2, 3, 2)  # tests/test_hip_processors.py
S_VID = 8 * 6 * 8
N_RANDOM = 48
RATIOS = {}  # (dtype name, gradient) -> list of e_hip / e_torch over the random launches


def _fro(x):
    return float(torch.linalg.norm(x.double().reshape(-1)))


def _errs(got, t16, ref):
    """(e_hip, e_torch), or None when the float64 gradient is exactly zero (then `got` must be exactly zero)"""
    n = _fro(ref)
    if n == 0.0:
        assert not got.any(), "gradient must be exactly zero"
        return None
    return _fro(got.double() - ref) / n, _fro(t16.double() - ref) / n


def _bound(name, got, t16, ref, what=""):
    e = _errs(got, t16, ref)
    if e is None:
        return None
    print(f"{what} {name}: e_hip {e[0]:.3e} e_torch {e[1]:.3e} ratio {e[0] / max(e[1], 1e-300):.3f}")
    assert e[0] <= 2.0 * e[1], f"{what} {name}: e_hip {e[0]:.3e} > 2 x e_torch {e[1]:.3e}"
    return e


def _reference_grads(kws_outs, q, k, v, dtype, weights_grad):
    """gradients of sum(out * weights_grad) through the restatement in `dtype`; kws_outs = [(keywords, buffer index)],
    weights_grad(bufs) -> the tensor whose sum with the buffers is the loss, as a list of per-buffer cotangents"""
    leaves = [x.detach().to(dtype).requires_grad_(True) for x in (q, k, v)]
    n_buf = 1 + max(i for _, i in kws_outs)
    bufs = [torch.zeros(q.shape, dtype=dtype, device=q.device) for _ in range(n_buf)]
    for kw, i in kws_outs:
        restate(kw, *leaves, bufs[i])
    cots = weights_grad(dtype)
    live = [(b, c) for b, c in zip(bufs, cots) if b.requires_grad]
    if not live:
        return [torch.zeros_like(x) for x in leaves], bufs
    grads = torch.autograd.grad([b for b, _ in live], leaves, [c for _, c in live], allow_unused=True)
    return [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)], bufs


@pytest.mark.parametrize("seed", range(N_RANDOM))
def test_random_launch_gradients(seed):
    from vorta_amd import ops
    rng = np.random.default_rng(1000 + seed)
    dtype = (torch.bfloat16, torch.float16)[seed % 2]
    L = RL.draw(rng, device_lengths=True, heads_dev=True)
    kw = RL.kwargs(L, dev())
    gen = torch.Generator(device="cpu").manual_seed(seed)
    shape = (L.H_buf, L.S, 128)
    q, k, v, d_o = (torch.randn(shape, generator=gen).to(dtype).to(dev()) for _ in range(4))
    w = torch.randn(L.H_buf, generator=gen).to(dtype).to(dev()) if seed % 4 < 2 else None
    out = torch.full(shape, RL.SENTINEL, dtype=dtype, device=dev())
    ops.attn_fwd(q, k, v, out, **kw)

    def cot(dt):
        g = d_o.to(dt)
        return [g if w is None else g * w.to(dt)[:, None, None]]

    ref, _ = _reference_grads([(kw, 0)], q, k, v, torch.float64, cot)
    t16, _ = _reference_grads([(kw, 0)], q, k, v, dtype, cot)
    zero = [torch.zeros(shape, dtype=torch.float32, device=dev()) for _ in range(3)]
    ops.attn_bwd(q, k, v, out, d_o, *zero, do_scale=w, **kw)
    sent = [torch.full(shape, 3.0, dtype=torch.float32, device=dev()) for _ in range(3)]
    ops.attn_bwd(q, k, v, out, d_o, *sent, do_scale=w, **kw)
    what = f"seed {seed} {RL.describe(L)}"
    qm, km = named_rows(kw, shape)
    for name, got, s, t, r in zip(("dq", "dk", "dv"), zero, sent, t16, ref):
        # rows and heads the launch does not name (dead slots, rows past q_valid, keys past n_kv, rows outside the tables)
        # must receive exactly 0.0
        untouched = ~(qm if name == "dq" else km).to(dev())
        assert not r[untouched].any()  # (the restatement agrees on which rows those are)
        assert not got[untouched].any(), f"{what}: {name} wrote rows the launch does not name"
        assert (s[untouched] == 3.0).all(), f"{what}: {name} disturbed the sentinel of unnamed rows"
        # the "added to" contract: sentinel + gradient.  dq has one writer per row: exact; dk / dv are sums of float atomics
        # (float32 at magnitude 3: half an ulp, 1.2e-7, per addition -- one for dq, one per query block for dk / dv)
        tol = 1e-6 if name == "dq" else 1e-5
        assert torch.allclose(s, got + 3.0, rtol=tol, atol=tol), f"{what}: {name} is not sentinel + gradient"
        e = _bound(name, got, t, r, what)
        if e is not None and e[1] > 0:
            RATIOS.setdefault((str(dtype).split(".")[-1], name), []).append(e[0] / e[1])


def test_accuracy_summary_written():
    """max / median of e_hip / e_torch over the random launches, per gradient and dtype (runs after them; the figures of
    profiles/attn_bwd_accuracy.txt come from here when VORTA_BWD_ACCURACY_OUT names a file)"""
    if not RATIOS:
        return  # (selected on its own: nothing to summarise)
    lines = [f"{dt} {name}: cases {len(r)} max {max(r):.3f} median {float(np.median(r)):.3f}"
             for (dt, name), r in sorted(RATIOS.items())]
    print("\n".join(lines))
    path = os.environ.get("VORTA_BWD_ACCURACY_OUT")
    if path:
        with open(path, "w") as f:
            f.write("e_hip / e_torch over the random launches of tests/test_hip_attention_bwd.py (bound: 2)\n" + "\n".join(lines) + "\n")
    assert all(max(r) <= 2.0 for r in RATIOS.values())


# ------------------------------------------------------------------------------------------------ soft mixture, end to end
def _mixture_case(model, dtype, golden, H=4, seed=5):
    from vorta_amd.routed import geometry_for
    t, te = (int(x) for x in golden("g8_eval_calls")["text"]) if model == "hunyuan" else (0, 0)
    geom = geometry_for(LATENT, TILE, WINDOW, GROUP, 0.5, dev())
    gen = torch.Generator(device="cpu").manual_seed(seed)
    shape = (1, H, S_VID + t, 128)
    q, k, v, G = (torch.randn(shape, generator=gen).to(dtype).to(dev()) for _ in range(4))
    sc = torch.softmax(torch.randn((1, H, 3), generator=gen), dim=-1).to(dtype).to(dev())
    return geom, t, te, q, k, v, sc, G


def _mixture_reference(launches, bufs, q, k, v, sc, G, dtype):
    """gradients of sum(mix(experts) * G) through the restatement of the RECORDED launches (the ranking is a constant)"""
    leaves = [x[0].detach().to(dtype).requires_grad_(True) for x in (q, k, v)]
    s = sc[0].detach().to(dtype).requires_grad_(True)
    outs = [torch.zeros(leaves[0].shape, dtype=dtype, device=q.device) for _ in range(3)]
    for c in launches:
        e = next(i for i, b in enumerate(bufs) if b.data_ptr() == c["out"].data_ptr())
        kw = {key: val for key, val in c.items() if key not in ("q", "k", "v", "out")}
        restate(kw, *leaves, outs[e])
    mixed = sum(s[:, e, None, None] * outs[e] for e in range(3))
    grads = torch.autograd.grad(mixed, leaves + [s], G[0].to(dtype))
    return grads, outs


@pytest.mark.parametrize("model", ["hunyuan", "wan"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_soft_mixture_autograd_end_to_end(model, dtype, golden):
    from vorta_amd.routed import (HeadRouting, routed_attention, soft_mixture_attention,
                                  soft_mixture_attention_autograd)
    geom, t, te, q, k, v, sc, G = _mixture_case(model, dtype, golden)
    H = q.shape[1]
    kwm = dict(model=model, text_len=t, text_valid=te)
    plain = soft_mixture_attention(q, k, v, sc, geom, **kwm)
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v, sc)]
    out = soft_mixture_attention_autograd(*leaves, geom, **kwm)
    assert torch.equal(out, plain)  # (a) the same bits as the forward-only operator
    (out * G).sum().backward()
    dq, dk, dv, dsc = (x.grad for x in leaves)
    # a separate forward: the three expert buffers and the launches as launched
    bufs, launches = [torch.empty_like(q) for _ in range(3)], []
    routed_attention(q, k, v, HeadRouting.every_head_everywhere(H, q.device), geom, expert_outs=bufs, fp8=False,
                     record=launches, **kwm)
    assert len(launches) == (4 if model == "hunyuan" else 3)
    bufs3 = [b[0] for b in bufs]
    # (b) dscores = <G[h], x_e[h]>: exact identity, the yardstick is the 16-bit dot product
    want = torch.stack([(G[0].double() * b.double()).sum((1, 2)) for b in bufs3], dim=1)
    t16 = torch.stack([(G[0] * b).sum((1, 2)) for b in bufs3], dim=1)
    _bound("dscores", dsc[0], t16, want, f"{model} {dtype}")
    assert dsc.shape == sc.shape and dsc.dtype == sc.dtype
    # (c) dq, dk, dv against float64 autograd through the SAME keep / drop lists and sliding tables
    ref, _ = _mixture_reference(launches, bufs3, q, k, v, sc, G, torch.float64)
    y16, _ = _mixture_reference(launches, bufs3, q, k, v, sc, G, dtype)
    for name, got, a, b in zip(("dq", "dk", "dv"), (dq, dk, dv), y16, ref):
        assert got.dtype == dtype and got.shape == q.shape
        _bound(name, got[0], a, b, f"{model} {dtype}")
    # (d) padded text rows take no gradient
    if t > te:
        for g in (dq, dk, dv):
            assert not g[:, :, S_VID + te:].any()


@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_dropped_coreset_margins_send_their_gradient_to_the_centre(model, golden):
    """coreset expert alone (scores 0, 1, 0) with a loss that only reads DROPPED margin rows: their own dq is zero, and the
    gradient reaches q, k, v through the centres the rows were copied from"""
    from vorta_amd.routed import soft_mixture_attention_autograd
    dtype = torch.float16
    geom, t, te, q, k, v, sc, G = _mixture_case(model, dtype, golden, seed=9)
    sc = torch.zeros_like(sc)
    sc[..., 1] = 1.0
    launches = []
    from vorta_amd.routed import HeadRouting, routed_attention
    bufs = [torch.empty_like(q) for _ in range(3)]
    routed_attention(q, k, v, HeadRouting.every_head_everywhere(q.shape[1], q.device), geom, expert_outs=bufs, fp8=False,
                     record=launches, model=model, text_len=t, text_valid=te)
    low = next(c for c in launches if c.get("dup_rows") is not None)
    drop, keep = low["dup_rows"].long(), low["q_rows"].long()  # (H, G, n_drop), (H, n_q)
    mask = torch.zeros(q.shape[1:3], dtype=torch.bool, device=q.device)
    mask.scatter_(1, drop.reshape(drop.shape[0], -1), True)
    G = G * mask[None, :, :, None]
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v, sc)]
    out = soft_mixture_attention_autograd(*leaves, geom, model=model, text_len=t, text_valid=te)
    (out * G).sum().backward()
    dq = leaves[0].grad[0]
    assert not dq[mask].any()  # a dropped row's query is never read
    centres = torch.zeros_like(mask)
    centres.scatter_(1, keep[:, :geom.G], True)
    assert dq[centres].any() and not dq[~centres].any()
    ref, _ = _mixture_reference(launches, [b[0] for b in bufs], q, k, v, sc, G, torch.float64)
    y16, _ = _mixture_reference(launches, [b[0] for b in bufs], q, k, v, sc, G, dtype)
    for name, got, a, b in zip(("dq", "dk", "dv"), [x.grad[0] for x in leaves[:3]], y16, ref):
        _bound(name, got, a, b, f"{model} coreset only")


def test_dense_attention_autograd():
    from vorta_amd.routed import dense_attention, dense_attention_autograd
    gen = torch.Generator(device="cpu").manual_seed(3)
    for dtype in (torch.bfloat16, torch.float16):
        q = torch.randn((1, 3, 200, 128), generator=gen).to(dtype).to(dev())
        k, v = (torch.randn((1, 3, 333, 128), generator=gen).to(dtype).to(dev()) for _ in range(2))
        G = torch.randn(q.shape, generator=gen).to(dtype).to(dev())
        leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
        out = dense_attention_autograd(*leaves, kv_valid=300, q_valid=190)
        assert torch.equal(out, dense_attention(q, k, v, kv_valid=300, q_valid=190))
        (out * G).sum().backward()

        def grads(dt):
            x = [a[0].detach().to(dt).requires_grad_(True) for a in (q, k, v)]
            p = torch.softmax(x[0] @ x[1][:, :300].transpose(1, 2) / 128 ** 0.5, dim=-1) @ x[2][:, :300]
            p = torch.cat([p[:, :190], torch.zeros_like(p[:, 190:])], dim=1)
            return torch.autograd.grad(p, x, G[0].to(dt))

        for name, got, a, b in zip(("dq", "dk", "dv"), leaves, grads(dtype), grads(torch.float64)):
            _bound(name, got.grad[0], a, b, f"dense {dtype}")
        assert not leaves[0].grad[:, :, 190:].any() and not leaves[1].grad[:, :, 300:].any()


# ------------------------------------------------------------------------------------------------ the torch operator
def test_torch_op_matches_and_passes_opcheck(golden):
    from vorta_amd import torch_ops  # noqa: F401
    from vorta_amd.routed import soft_mixture_attention_autograd
    dtype = torch.bfloat16
    geom, t, te, q, k, v, sc, G = _mixture_case("hunyuan", dtype, golden, H=2)
    geo = dict(latent=list(LATENT), tile=list(TILE), window=list(WINDOW), group=list(GROUP), rate=0.5)
    a = [x.clone().requires_grad_(True) for x in (q, k, v, sc)]
    b = [x.clone().requires_grad_(True) for x in (q, k, v, sc)]
    out_a = torch.ops.vorta.soft_mixture_attention_grad(*a, model="hunyuan", text_len=t, text_valid=te, **geo)
    out_b = soft_mixture_attention_autograd(*b, geom, model="hunyuan", text_len=t, text_valid=te)
    assert torch.equal(out_a, out_b)
    (out_a * G).sum().backward()
    (out_b * G).sum().backward()
    assert torch.equal(a[0].grad, b[0].grad) and torch.equal(a[3].grad, b[3].grad)  # dq, dscores: reproducible
    for x, y in zip(a[1:3], b[1:3]):  # dk, dv: float atomics, equal up to the last 16-bit place
        assert _fro(x.grad.double() - y.grad.double()) <= 2.0 ** -7 * _fro(y.grad)
    args = tuple(x.detach().clone().requires_grad_(True) for x in (q, k, v, sc))
    torch.library.opcheck(torch.ops.vorta.soft_mixture_attention_grad.default, args,
                          dict(model="hunyuan", text_len=t, text_valid=te, **geo),
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
