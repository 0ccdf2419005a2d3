"""Helpers of tests/test_hip_sp_soft_mixture.py and tests/_rccl_single_rank_soft_mixture.py: the cases of the soft mixture
under sequence parallelism and their float64 references.

Geometry: the smallest latent whose every dimension is a multiple of both the tile (2,3,4) and the coreset window (2,3,2),
with S a multiple of 4 and S/P >= 128 at P = 4 (two 64-key blocks and one full 128-row query workgroup per shard), and --
as every geometry of the existing tests -- at least two tiles per dimension: (12, 6, 8), S = 576; S/P = 288 and 144, neither
a multiple of the 128 query rows of a workgroup.  Hunyuan: T = 8 text rows, 5 valid; Wan: no text rows."""
import os
import sys

import numpy as np
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

LATENT, TILE, WINDOW, GROUP, RATE = (12, 6, 8), (2, 3, 4), (3, 3, 3), (2, 3, 2), 0.5
S, D = 12 * 6 * 8, 128
T_HY, TE_HY = 8, 5


def dev():
    return torch.device("cuda:0")


def rel_err(a, b) -> float:
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def text_of(model: str):
    return (T_HY, TE_HY) if model == "hunyuan" else (0, 0)


def operator_case(model: str, H: int, dtype, seed: int = 3):
    """global q, k, v (1, H, S + T, D), scores (1, H, 3), cotangent (1, S + T, H, D): the same on every rank"""
    T, _ = text_of(model)
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn((1, H, S + T, D), generator=g).to(dtype).to(dev()) for _ in range(3))
    sc = torch.softmax(torch.randn((1, H, 3), generator=g), dim=-1).to(dtype).to(dev())
    cot = torch.randn((1, S + T, H, D), generator=g).to(dtype).to(dev())
    return q, k, v, sc, cot


def geometry_kw():
    from vorta_amd.attention import get_group_info
    return dict(lowres_group_info=get_group_info(LATENT, GROUP, RATE, dev()), window_size=WINDOW, tile_size=TILE,
                latent_shape=LATENT)


def shard(x, rank: int, P: int, n_video: int = S, dim: int = 2):
    """the rank's sequence shard of a global tensor whose `dim` is [video | text]: its video rows, then all text rows"""
    Sl = n_video // P
    return torch.cat([x.narrow(dim, rank * Sl, Sl), x.narrow(dim, n_video, x.shape[dim] - n_video)], dim=dim).contiguous()


class RecordSp:
    """the launches of the sequence-parallel soft mixture as launched, by spying on the routed_attention the operator calls"""

    def __enter__(self):
        import vorta_amd.attention._sp as sp
        self.sp, self.stock, self.calls = sp, sp.routed_attention, []

        def spy(*a, **kw):
            if kw.get("record") is not None:
                self.calls.append((kw["record"], list(kw["expert_outs"]), a[4].row_map))
            return self.stock(*a, **kw)

        sp.routed_attention = spy
        return self

    def __exit__(self, *exc):
        self.sp.routed_attention = self.stock


_TABLES = ("q_rows", "kv_rows", "dup_rows")
_SCALARS = ("n_q", "n_kv", "q_valid", "n_heads", "q_group_len", "kv_rows_stride_g", "n_dup_pos", "scale", "n_key_lists", "tag")


def globalize(call, head0: int):
    """one rank's recorded launches -> plain dictionaries in GLOBAL coordinates (numpy): rows of the receive layout become
    tokens (the inverse of the row map), local head slots become heads, the output buffer becomes its expert's index"""
    launches, ebufs, rm = call
    rm = rm.long().cpu()
    inv = torch.full((int(rm.max()) + 1,), -1, dtype=torch.int64)
    inv[rm] = torch.arange(rm.numel())
    ptrs = [b.data_ptr() for b in ebufs]
    out = []
    for c in launches:
        g = {k: c[k] for k in _SCALARS if c.get(k) is not None}
        assert c.get("n_heads_dev") is None and c.get("n_kv_dev") is None and c.get("q_valid_dev") is None
        assert not c.get("q_row_offset") and not c.get("kv_row_offset")
        for k in _TABLES:
            if c.get(k) is not None:
                t = inv[c[k].long().cpu()]
                assert int(t.min()) >= 0, k
                g[k] = t.numpy()
        if c.get("q_block_table") is not None:
            g["q_block_table"] = c["q_block_table"].cpu().numpy()
        hl = c["head_list"].long().cpu() if c.get("head_list") is not None else torch.arange(c["n_heads"])
        g["head_list"] = (hl + head0).numpy()
        g["expert"] = ptrs.index(c["out"].data_ptr())
        out.append(g)
    return out


def as_launches(globalized):
    """(launches, bufs) as tests/test_hip_processors_grad.py `_mixture` reads them; tables back as tensors"""
    bufs = [torch.empty(1) for _ in range(3)]
    launches = []
    for g in globalized:
        c = {k: (torch.as_tensor(v) if isinstance(v, np.ndarray) else v) for k, v in g.items() if k != "expert"}
        c["out"] = bufs[g["expert"]]
        launches.append(c)
    return launches, bufs


def restated_mixture(q, k, v, sc, globalized):
    """tests/_attn_restate.py over the launches, then the mix: q, k, v (H, N, D), sc (1, H, 3), any dtype, differentiable"""
    from _attn_restate import restate
    outs = [torch.zeros(q.shape, dtype=q.dtype, device=q.device) for _ in range(3)]
    launches, _ = as_launches(globalized)
    for c, g in zip(launches, globalized):
        restate({key: val for key, val in c.items() if key != "out"}, q, k, v, outs[g["expert"]])
    return sum(sc[0][:, e, None, None] * outs[e] for e in range(3))


def reference_grads(q, k, v, sc, cot, globalized, dt):
    """(dq, dk, dv (H, N, D), dscores (1, H, 3), out (H, N, D)) of sum(out * cot) through the restatement in dtype `dt`"""
    L = [x.detach().to(dt).requires_grad_(True) for x in (q[0], k[0], v[0], sc)]
    o = restated_mixture(*L, globalized)
    g = torch.autograd.grad((o * cot[0].transpose(0, 1).to(dt)).sum(), L)
    return g, o.detach()


def oracle_forward(model, q, k, v, sc):
    from oracle import vorta_oracle as O
    T, te = text_of(model)
    f64 = lambda t: t.detach().double().cpu().numpy()  # noqa: E731
    return O.soft_mixture_attention(f64(q), f64(k), f64(v), f64(sc), model=model, latent=LATENT, tile=TILE, window=WINDOW,
                                    gi=O.group_info(LATENT, GROUP, RATE), t_text=T, t_eff=te)


def single_process_forward(model, q, k, v, sc):
    from vorta_amd.routed import geometry_for, soft_mixture_attention
    T, te = text_of(model)
    geom = geometry_for(LATENT, TILE, WINDOW, GROUP, RATE, dev())
    return soft_mixture_attention(q, k, v, sc, geom, model=model, text_len=T, text_valid=te)
