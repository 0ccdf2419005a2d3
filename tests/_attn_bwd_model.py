"""The yardstick of the structured-input backward tests: a ROUNDING MODEL of the attention backward, and the input families
it is measured on (tests/test_host_backward_model.py, tests/test_hip_attention_bwd_structured.py).

`model_grads` is float64 attention backward of one launch dictionary, walked with the geometry of tests/_attn_restate.py, with
exactly the three roundings to 16 bits that the kernels make by design and that can be pointed to in their source:

    g_eff = round16((d_o[row] + sum d_o[dup rows]) * w[head])   csrc/attn_bwd_kmajor.h:84, csrc/attn_bwd.hip:147
    P16   = round16(P), dS16 = round16(dS)                       csrc/attn_bwd.hip:306-320, csrc/attn_bwd_kmajor.h:453-454

    dV += P16^T g_eff,  dQ += scale dS16 K,  dK += scale dS16^T Q      (dS = P (dP - delta), dP = g_eff V^T, delta = sum_j P dP)

With round16=False it is plain float64 attention backward, which tests/test_host_backward_model.py pins against float64
autograd through the restatement.  Nothing here reads the library."""
import functools
import math

import numpy as np
import torch

import _random_launch as RL
import _structured_inputs as SI
from _attn_restate import launch_geometry, restate

LATENT = (8, 6, 8)
S_VID = 8 * 6 * 8
FAMILIES = ("white", "local", "redundant", "shift_up", "shift_down", "late_key", "common_cotangent")
DTYPES = (torch.bfloat16, torch.float16)
LATE_KEYS = ((5, 300, .5), (40, 350, 1.), (77, 383, 3.), (130, 200, .25))  # (row, key, b): k[key] = b q[row]
# the two gather launches: seeds of RL.draw(default_rng(seed), H_buf=2, S=400), chosen by their geometry alone (see
# `launch`): both have live heads, a non-empty q_valid and more than one 64-key block; between them a dead head slot, a block
# table with groups of different lengths, row tables, duplicate rows and both device lengths
#   24: one live head of two, a 128-row block table over three groups of 51 / 112 / 39 queries with their own lists of 228
#       keys, duplicate rows at 153 positions, a device n_kv
#    9: both heads, 268 scattered queries on 312 contiguous keys (two 256-key blocks), a device q_valid of 187 in mid
#       slice, duplicate rows at 43 positions
GATHER_SEEDS = {"gather_a": 24, "gather_b": 9}
LAUNCHES = ("dense", "gather_a", "gather_b")


def dtype_name(dtype):
    return str(dtype).split(".")[-1]


def _cpu(t):
    return None if t is None else t.detach().cpu().long()


def _walk(kw, H):
    """(slot, head, query rows of the launch's positions, [(first, end, key rows)] per group segment) per live head"""
    heads, groups, n_kv, q_valid = launch_geometry(kw, H)
    q_rows, kv_rows = _cpu(kw.get("q_rows")), _cpu(kw.get("kv_rows"))
    sg = kw.get("kv_rows_stride_g", 0)
    for y, h in enumerate(heads):
        if q_rows is None:
            qr = torch.arange(kw.get("q_row_offset", 0), kw.get("q_row_offset", 0) + kw["n_q"])
        else:
            qr = q_rows[y] if q_rows.dim() == 2 else q_rows
        segs = []
        for g, a, b in groups:
            if b <= a:
                continue
            if kv_rows is None:
                keys = torch.arange(kw.get("kv_row_offset", 0), kw.get("kv_row_offset", 0) + n_kv)
            elif sg > 0:
                keys = kv_rows.reshape(-1)[g * sg: g * sg + n_kv]
            else:
                keys = (kv_rows[y] if kv_rows.dim() == 2 else kv_rows)[:n_kv]
            segs.append((a, b, keys))
        yield y, h, qr, segs


def model_grads(kw, q, k, v, d_o, w, dtype, round16=True, work=torch.float64):
    """(dq, dk, dv, lse, delta) of one launch: dq / dk / dv (H,S,D), lse (natural units) and delta (head slots, n_q) with NaN at
    positions the launch does not cover; computed in `work` (float64: the model; float32 with round16=False: a plain
    float32 backward), returned in float64.  q, k, v, d_o: (H,S,D) of any dtype, w: (H,) weights per head id or None"""
    r16 = (lambda x: x.to(dtype).to(work)) if round16 else (lambda x: x)
    q, k, v, g = (x.detach().cpu().to(work) for x in (q, k, v, d_o))
    w = None if w is None else w.detach().cpu().to(work)
    H = q.shape[0]
    heads, _, _, q_valid = launch_geometry(kw, H)
    scale = kw.get("scale") or 1.0 / math.sqrt(q.shape[-1])
    dup = _cpu(kw.get("dup_rows"))
    dq, dk, dv = (torch.zeros_like(q) for _ in range(3))
    lse = torch.full((len(heads), kw["n_q"]), float("nan"), dtype=work)
    delta = lse.clone()
    for y, h, qr, segs in _walk(kw, H):
        g_eff = g[h, qr].clone()
        if dup is not None:
            dr = dup[y] if dup.dim() == 3 else dup
            npos = kw.get("n_dup_pos", 0) or dr.shape[0]
            g_eff[:npos] += g[h, dr[:npos]].sum(1)
        if w is not None:
            g_eff = g_eff * w[h]
        g_eff = r16(g_eff)
        g_eff[q_valid:] = 0
        for a, b, keys in segs:
            rows, K, V, G = qr[a:b], k[h, keys], v[h, keys], g_eff[a:b]
            Q = q[h, rows]
            s = (Q @ K.t()) * scale
            P = torch.softmax(s, dim=-1)
            dP = G @ V.t()
            dl = (P * dP).sum(-1)
            dS = P * (dP - dl[:, None])
            P16, dS16 = r16(P), r16(dS)
            dv[h].index_add_(0, keys, P16.t() @ G)
            dq[h].index_add_(0, rows, scale * (dS16 @ K))
            dk[h].index_add_(0, keys, scale * (dS16.t() @ Q))
            lse[y, a:b] = torch.logsumexp(s, dim=-1)
            delta[y, a:b] = dl
    return tuple(x.double() for x in (dq, dk, dv, lse, delta))


def score_abs_sums(kw, q, k):
    """max_j sum_d |q_d k_jd| per (head slot, position) in float64 (NaN where the launch covers nothing): what bounds the
    rounding error of a float32 dot product of length D"""
    q, k = q.detach().cpu().double().abs(), k.detach().cpu().double().abs()
    heads = launch_geometry(kw, q.shape[0])[0]
    out = torch.full((len(heads), kw["n_q"]), float("nan"), dtype=torch.float64)
    for y, h, qr, segs in _walk(kw, q.shape[0]):
        for a, b, keys in segs:
            out[y, a:b] = (q[h, qr[a:b]] @ k[h, keys].t()).max(-1).values
    return out


def autograd_grads(kw, q, k, v, d_o, w, dt):
    """(dq, dk, dv) of sum(out * d_o * w) by torch autograd through the restatement, everything in `dt`, on the CPU"""
    leaves = [x.detach().cpu().to(dt).requires_grad_(True) for x in (q, k, v)]
    out = restate(kw, *leaves, torch.zeros(q.shape, dtype=dt))
    if not out.requires_grad:
        return [torch.zeros_like(x) for x in leaves]
    cot = d_o.detach().cpu().to(dt)
    if w is not None:
        cot = cot * w.detach().cpu().to(dt)[:, None, None]
    grads = torch.autograd.grad(out, leaves, cot, allow_unused=True)
    return [torch.zeros_like(x) if g is None else g for g, x in zip(grads, leaves)]


def fro(x):
    return float(torch.linalg.norm(x.double().reshape(-1)))


# ----------------------------------------------------------------------------------------------------------- the inputs
def family(name, H, S, dtype, seed=7):
    """(q, k, v, d_o) of one input family as (H,S,128) CPU tensors rounded to `dtype`: the structure sits on the first 384
    rows (latent 8 x 6 x 8), rows past them are a white text tail"""
    assert S >= S_VID and name in FAMILIES
    gen = torch.Generator(device="cpu").manual_seed(seed)
    white = lambda *shape: torch.randn(shape, generator=gen)  # noqa: E731
    q, k, v, d_o = (white(H, S, 128) for _ in range(4))
    for h in range(H):
        if name == "local":
            q[h, :S_VID], k[h, :S_VID], v[h, :S_VID] = SI.local_head(LATENT, (0.75, 1.0, 1.34), 16.0, 0.1, gen, "cpu")
        elif name == "redundant":
            q[h, :S_VID], k[h, :S_VID], v[h, :S_VID] = SI.redundant_head(LATENT, (2, 3, 2), 0.05, gen, "cpu")
    if name == "shift_up":
        q, k = q + 3, k + 3
    elif name == "shift_down":
        q, k = q + 3, k - 3
    elif name == "late_key":
        for row, key, b in LATE_KEYS:
            k[:, key] = b * q[:, row]
    elif name == "common_cotangent":
        d_o = d_o + 4
    return tuple(x.to(dtype) for x in (q, k, v, d_o))


def launch(name, device="cpu"):
    """(H, S, launch keywords with their tables on `device`, with a do_scale or not) of one of LAUNCHES"""
    if name == "dense":
        return 1, S_VID, dict(n_q=S_VID, n_kv=S_VID), False
    L = RL.draw(np.random.default_rng(GATHER_SEEDS[name]), H_buf=2, S=400)
    return L.H_buf, L.S, RL.kwargs(L, device), True


@functools.lru_cache(maxsize=None)
def case(fam, dtype, which):
    """everything the tests need of one (family, dtype, launch), computed once on the CPU and left unchanged: the inputs,
    the float64 gradients and statistics, the model's, float32 autograd's and 16-bit autograd's"""
    H, S, kw, weighted = launch(which)
    q, k, v, d_o = family(fam, H, S, dtype)
    w = torch.randn(H, generator=torch.Generator(device="cpu").manual_seed(11)).to(dtype) if weighted else None
    f64 = model_grads(kw, q, k, v, d_o, w, dtype, round16=False)
    model = model_grads(kw, q, k, v, d_o, w, dtype)
    f32 = autograd_grads(kw, q, k, v, d_o, w, torch.float32)
    f32_delta = model_grads(kw, q, k, v, d_o, w, dtype, round16=False, work=torch.float32)[4]
    t16 = autograd_grads(kw, q, k, v, d_o, w, dtype)
    return dict(H=H, S=S, kw=kw, q=q, k=k, v=v, d_o=d_o, w=w, f64=f64, model=model, f32=f32, f32_delta=f32_delta, t16=t16,
                abs_sums=score_abs_sums(kw, q, k))


def rel_errors(c):
    """{gradient: (e_model, e_f32, e_torch16)} relative Frobenius errors against float64, None for a zero float64 gradient"""
    out = {}
    for i, name in enumerate(("dq", "dk", "dv")):
        n = fro(c["f64"][i])
        out[name] = None if n == 0.0 else tuple(fro(x[i].double() - c["f64"][i]) / n for x in (c["model"], c["f32"], c["t16"]))
    return out
