"""GPU: the key-major attention backward (vorta_attn_bwd_stats + vorta_attn_bwd_kmajor) against torch autograd in float64 on
the plain restatement of tests/_attn_restate.py -- the yardstick and the rule of tests/test_hip_attention_bwd.py:

    e_hip <= 2 e_torch per gradient, with e_torch the error of torch's own 16-bit autograd on the same restatement, and a
    gradient whose float64 norm is exactly zero must be exactly zero.

The statistics are held to the same rule: lse2 ln 2 against torch.logsumexp of the float64 scores and delta against the float64
sum_j P dP, with the same quantities computed by torch in the launch's dtype as the yardstick.

Measured on an MI355X (profiles/attn_bwd_key_major_accuracy.txt): e_hip / e_torch 0.35-0.41 in the median and at most 0.77 for
dq / dk / dv over the random launches, 0.27-0.36 for delta and under 0.001 for lse2."""
import math
import os

import numpy as np
import pytest
import torch

import _random_launch as RL
import test_hip_attention_bwd as B
from _attn_restate import launch_geometry, named_rows
from _util import dev

pytestmark = pytest.mark.gpu

RATIOS = {}  # (dtype name, quantity) -> list of e_hip / e_torch


def _name(dtype):
    return str(dtype).split(".")[-1]


def _key_major(q, k, v, out, d_o, bufs, w, kw, stats=None):
    from vorta_amd import ops
    if stats is None:
        stats = ops.attn_bwd_stats(q, k, v, out, d_o, do_scale=w, **kw)
    ops.attn_bwd_key_major(q, k, v, out, d_o, *bufs, stats, do_scale=w, **kw)
    return stats


def _inputs(shape, dtype, seed, weight):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    q, k, v, d_o = (torch.randn(shape, generator=gen).to(dtype).to(dev()) for _ in range(4))
    w = torch.randn(shape[0], generator=gen).to(dtype).to(dev()) if weight else None
    return q, k, v, d_o, w


def _references(kw, q, k, v, d_o, w, dtype):
    def cot(dt):
        g = d_o.to(dt)
        return [g if w is None else g * w.to(dt)[:, None, None]]

    ref, _ = B._reference_grads([(kw, 0)], q, k, v, torch.float64, cot)
    t16, _ = B._reference_grads([(kw, 0)], q, k, v, dtype, cot)
    return ref, t16


def _check_launch(kw, shape, dtype, seed, weight, what, ratios=None):
    """one launch through both passes: the bound, exact zeros where the launch names nothing, the "added to" contract"""
    from vorta_amd import ops
    q, k, v, d_o, w = _inputs(shape, dtype, seed, weight)
    out = torch.full(shape, RL.SENTINEL, dtype=dtype, device=dev())
    ops.attn_fwd(q, k, v, out, **kw)
    ref, t16 = _references(kw, q, k, v, d_o, w, dtype)
    zero = [torch.zeros(shape, dtype=torch.float32, device=dev()) for _ in range(3)]
    stats = _key_major(q, k, v, out, d_o, zero, w, kw)
    sent = [torch.full(shape, 3.0, dtype=torch.float32, device=dev()) for _ in range(3)]
    _key_major(q, k, v, out, d_o, sent, w, kw, stats)
    qm, km = named_rows(kw, shape)
    for name, got, s, t, r in zip(("dq", "dk", "dv"), zero, sent, t16, ref):
        untouched = ~(qm if name == "dq" else km).to(dev())
        assert not r[untouched].any()  # (the restatement agrees on which rows those are)
        assert not got[untouched].any(), f"{what}: {name} wrote rows the launch does not name"
        assert (s[untouched] == 3.0).all(), f"{what}: {name} disturbed the sentinel of unnamed rows"
        # all three are sums of float atomics here (float32 at magnitude 3: half an ulp, 1.2e-7, per addition -- one per
        # key block for dq, one per group and launch for dk / dv): the tolerance tests/test_hip_attention_bwd.py gives dk / dv
        assert torch.allclose(s, got + 3.0, rtol=1e-5, atol=1e-5), f"{what}: {name} is not sentinel + gradient"
        e = B._bound(name, got, t, r, what)
        if ratios is not None and e is not None and e[1] > 0:
            ratios.setdefault((_name(dtype), name), []).append(e[0] / e[1])


# ------------------------------------------------------------------------------------------------------- random launches
@pytest.mark.parametrize("seed", range(B.N_RANDOM))
def test_random_launch_gradients(seed):
    rng = np.random.default_rng(1000 + seed)
    dtype = (torch.bfloat16, torch.float16)[seed % 2]
    L = RL.draw(rng, device_lengths=True, heads_dev=True)
    kw = RL.kwargs(L, dev())
    _check_launch(kw, (L.H_buf, L.S, 128), dtype, seed, seed % 4 < 2, f"seed {seed} {RL.describe(L)}", RATIOS)


# ---------------------------------------------------------------------------------------------------- named small shapes
def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int32), device=dev())


def _two_lists(n_kv, first=0, shift=100):
    """two key lists of n_kv rows that share the rows [shift, n_kv) of the first"""
    return _t(np.stack([np.arange(first, first + n_kv), np.arange(first + shift, first + shift + n_kv)]))


def _named_shapes():
    S = 480
    cases = {}
    for n_kv in (1, 63, 256, 257, 300):  # under one key block; one full block; a one-key second block; a ragged second block
        cases[f"n_kv_{n_kv}"] = (2, S, dict(n_q=40, n_kv=n_kv, q_row_offset=7, kv_row_offset=3))
    for n_q in (31, 33):  # a ragged slice
        cases[f"n_q_{n_q}"] = (1, S, dict(n_q=n_q, n_kv=100))
    # a group shorter than one slice next to a longer one; key lists that overlap in rows 100..149 and not elsewhere
    cases["short_group"] = (2, S, dict(n_q=70, q_group_len=50, n_kv=150, kv_rows=_two_lists(150), kv_rows_stride_g=150))
    for br, rows in ((128, [(0, 0, 100), (1, 100, 228), (0, 228, 300), (1, 300, 340)]),
                     (256, [(1, 0, 200), (0, 200, 456), (1, 456, 470)])):  # the rows of two groups interleave
        cases[f"table_{br}"] = (2, S, dict(n_q=rows[-1][2], n_kv=270, kv_rows=_two_lists(270, first=5), kv_rows_stride_g=270,
                                           q_block_table=_t(rows), n_key_lists=2, block_rows=br,
                                           q_rows=_t(np.random.default_rng(br).permutation(S)[:rows[-1][2]])))
    dup = np.arange(300, 320).reshape(10, 2)
    cases["dup_rows_2"] = (2, S, dict(n_q=40, n_kv=90, q_rows=_t(np.arange(40) * 3), dup_rows=_t(dup), n_dup_pos=10))
    cases["q_valid_mid_slice"] = (1, S, dict(n_q=70, n_kv=300, q_valid=45))
    cases["q_valid_0"] = (1, S, dict(n_q=70, n_kv=300, q_valid=0))
    cases["n_heads_dev_0"] = (2, S, dict(n_q=40, n_kv=70, n_heads_dev=torch.zeros(1, dtype=torch.int32, device=dev())))
    cases["head_list_skips"] = (4, S, dict(n_q=40, n_kv=270, head_list=_t([3, 1]), n_heads=2))
    return cases


NAMED = ("n_kv_1", "n_kv_63", "n_kv_256", "n_kv_257", "n_kv_300", "n_q_31", "n_q_33", "short_group", "table_128", "table_256",
         "dup_rows_2", "q_valid_mid_slice", "q_valid_0", "n_heads_dev_0", "head_list_skips")


@pytest.mark.parametrize("case", NAMED)
def test_named_small_shapes(case):
    H, S, kw = _named_shapes()[case]
    for i, dtype in enumerate((torch.bfloat16, torch.float16)):
        _check_launch(kw, (H, S, 128), dtype, 50 + i, True, f"{case} {_name(dtype)}")


# ------------------------------------------------------------------------------------------------------ statistics alone
def _stats_reference(kw, q, k, v, d_o, w, dt):
    """(lse in natural units, delta) per (head slot, position) from the restatement's geometry, computed in `dt`; positions
    the launch does not cover are NaN"""
    H = q.shape[0]
    heads, groups, n_kv, q_valid = launch_geometry(kw, H)
    scale = kw.get("scale") or 1.0 / math.sqrt(q.shape[-1])
    cpu = lambda t: None if t is None else t.detach().cpu().long()  # noqa: E731
    q_rows, kv_rows, dup = cpu(kw.get("q_rows")), cpu(kw.get("kv_rows")), cpu(kw.get("dup_rows"))
    sg = kw.get("kv_rows_stride_g", 0)
    lse = torch.full((len(heads), kw["n_q"]), float("nan"), dtype=torch.float64)
    delta = lse.clone()
    q, k, v, g = (x.to(dt) for x in (q, k, v, d_o))
    for y, h in enumerate(heads):
        qr = torch.arange(kw.get("q_row_offset", 0), kw.get("q_row_offset", 0) + kw["n_q"]) if q_rows is None else q_rows
        g_eff = g[h, qr.to(q.device)]
        if dup is not None:
            npos = kw.get("n_dup_pos", 0) or dup.shape[0]
            g_eff = g_eff.clone()
            g_eff[:npos] = g_eff[:npos] + g[h, dup[:npos].to(q.device)].sum(1)
        if w is not None:
            g_eff = g_eff * w.to(dt)[h]
        g_eff[q_valid:] = 0
        for grp, a, b in groups:
            if kv_rows is None:
                keys = torch.arange(kw.get("kv_row_offset", 0), kw.get("kv_row_offset", 0) + n_kv)
            else:
                keys = kv_rows.reshape(-1)[grp * sg: grp * sg + n_kv]
            keys = keys.to(q.device)
            s = (q[h, qr[a:b].to(q.device)] @ k[h, keys].transpose(0, 1)) * scale
            lse[y, a:b] = torch.logsumexp(s, dim=-1).double().cpu()
            delta[y, a:b] = (torch.softmax(s, dim=-1) * (g_eff[a:b] @ v[h, keys].transpose(0, 1))).sum(-1).double().cpu()
    return lse, delta


@pytest.mark.parametrize("case", ["n_kv_300", "table_128", "dup_rows_2"])
def test_statistics_alone(case):
    from vorta_amd import ops
    H, S, kw = _named_shapes()[case]
    for i, dtype in enumerate((torch.bfloat16, torch.float16)):
        q, k, v, d_o, w = _inputs((H, S, 128), dtype, 70 + i, True)
        out = torch.empty_like(q)
        ops.attn_fwd(q, k, v, out, **kw)
        stats = ops.attn_bwd_stats(q, k, v, out, d_o, do_scale=w, **kw).double().cpu()
        assert tuple(stats.shape) == ops.attn_bwd_stats_shape(H if kw.get("n_heads") is None else kw["n_heads"], kw["n_q"])
        want = _stats_reference(kw, q, k, v, d_o, w, torch.float64)
        t16 = _stats_reference(kw, q, k, v, d_o, w, dtype)
        covered = ~torch.isnan(want[0])
        assert covered.any()
        for name, got, t, r in zip(("lse", "delta"), (stats[..., 0] * math.log(2.0), stats[..., 1]), t16, want):
            n = B._fro(r[covered])
            e_hip, e_t = B._fro(got[covered] - r[covered]) / n, B._fro(t[covered] - r[covered]) / n
            print(f"{case} {_name(dtype)} {name}: e_hip {e_hip:.3e} e_torch {e_t:.3e} ratio {e_hip / max(e_t, 1e-300):.4f}")
            RATIOS.setdefault((_name(dtype), "stats " + name), []).append(e_hip / max(e_t, 1e-300))
            assert e_hip <= 2.0 * e_t, f"{case} {name}: e_hip {e_hip:.3e} > 2 x e_torch {e_t:.3e}"


# ---------------------------------------------------------------------------------------- agreement of the two algorithms
@pytest.mark.parametrize("seed", range(6))
def test_key_major_agrees_with_query_major(seed):
    """the two algorithms differ by no more than the sum of their errors against float64 (a wrong scale, a missing weight or
    a missing duplicate row that both pass loosely shows here).  In one norm this is the triangle inequality, so the figures
    that matter are the printed ones: the distance against each algorithm's own error."""
    from vorta_amd import ops
    rng = np.random.default_rng(1000 + seed)
    dtype = (torch.bfloat16, torch.float16)[seed % 2]
    L = RL.draw(rng, device_lengths=True, heads_dev=True)
    kw = RL.kwargs(L, dev())
    shape = (L.H_buf, L.S, 128)
    q, k, v, d_o, w = _inputs(shape, dtype, seed, True)
    out = torch.empty(shape, dtype=dtype, device=dev())
    ops.attn_fwd(q, k, v, out, **kw)
    ref, _ = _references(kw, q, k, v, d_o, w, dtype)
    km = [torch.zeros(shape, dtype=torch.float32, device=dev()) for _ in range(3)]
    qm = [torch.zeros(shape, dtype=torch.float32, device=dev()) for _ in range(3)]
    _key_major(q, k, v, out, d_o, km, w, kw)
    ops.attn_bwd(q, k, v, out, d_o, *qm, do_scale=w, **kw)
    for name, a, b, r in zip(("dq", "dk", "dv"), km, qm, ref):
        apart, e_a, e_b = B._fro(a.double() - b.double()), B._fro(a.double() - r), B._fro(b.double() - r)
        print(f"seed {seed} {name}: apart {apart:.3e} e_key_major {e_a:.3e} e_query_major {e_b:.3e}")
        assert apart <= e_a + e_b, f"seed {seed} {name}: the algorithms are {apart:.3e} apart, errors {e_a:.3e} + {e_b:.3e}"


# ------------------------------------------------------------------------------------------------ soft mixture, end to end
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_soft_mixture_autograd_key_major(model, dtype, golden):
    from vorta_amd.routed import HeadRouting, routed_attention, soft_mixture_attention_autograd
    geom, t, te, q, k, v, sc, G = B._mixture_case(model, dtype, golden)
    H = q.shape[1]
    kwm = dict(model=model, text_len=t, text_valid=te)
    with torch.no_grad():
        by_query = soft_mixture_attention_autograd(q, k, v, sc, geom, backward="query_major", **kwm)
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v, sc)]
    out = soft_mixture_attention_autograd(*leaves, geom, backward="key_major", **kwm)
    assert torch.equal(out, by_query)  # the forward does not depend on the backward's algorithm
    (out * G).sum().backward()
    dq, dk, dv, dsc = (x.grad for x in leaves)
    bufs, launches = [torch.empty_like(q) for _ in range(3)], []
    routed_attention(q, k, v, HeadRouting.every_head_everywhere(H, q.device), geom, expert_outs=bufs, fp8=False,
                     record=launches, **kwm)
    bufs3 = [b[0] for b in bufs]
    want = torch.stack([(G[0].double() * b.double()).sum((1, 2)) for b in bufs3], dim=1)
    t16 = torch.stack([(G[0] * b).sum((1, 2)) for b in bufs3], dim=1)
    B._bound("dscores", dsc[0], t16, want, f"key_major {model} {dtype}")
    ref, _ = B._mixture_reference(launches, bufs3, q, k, v, sc, G, torch.float64)
    y16, _ = B._mixture_reference(launches, bufs3, q, k, v, sc, G, dtype)
    for name, got, a, b in zip(("dq", "dk", "dv"), (dq, dk, dv), y16, ref):
        assert got.dtype == dtype and got.shape == q.shape
        B._bound(name, got[0], a, b, f"key_major {model} {dtype}")
    if t > te:  # padded text rows take no gradient
        for g in (dq, dk, dv):
            assert not g[:, :, B.S_VID + te:].any()


def test_dense_attention_autograd_key_major():
    from vorta_amd.routed import dense_attention, dense_attention_autograd
    gen = torch.Generator(device="cpu").manual_seed(3)
    for dtype in (torch.bfloat16, torch.float16):
        q = torch.randn((1, 3, 200, 128), generator=gen).to(dtype).to(dev())
        k, v = (torch.randn((1, 3, 333, 128), generator=gen).to(dtype).to(dev()) for _ in range(2))
        G = torch.randn(q.shape, generator=gen).to(dtype).to(dev())
        leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
        out = dense_attention_autograd(*leaves, kv_valid=300, q_valid=190, backward="key_major")
        assert torch.equal(out, dense_attention(q, k, v, kv_valid=300, q_valid=190))
        (out * G).sum().backward()

        def grads(dt):
            x = [a[0].detach().to(dt).requires_grad_(True) for a in (q, k, v)]
            p = torch.softmax(x[0] @ x[1][:, :300].transpose(1, 2) / 128 ** 0.5, dim=-1) @ x[2][:, :300]
            p = torch.cat([p[:, :190], torch.zeros_like(p[:, 190:])], dim=1)
            return torch.autograd.grad(p, x, G[0].to(dt))

        for name, got, a, b in zip(("dq", "dk", "dv"), leaves, grads(dtype), grads(torch.float64)):
            B._bound(name, got.grad[0], a, b, f"key_major dense {dtype}")
        assert not leaves[0].grad[:, :, 190:].any() and not leaves[1].grad[:, :, 300:].any()


# ------------------------------------------------------------------------------------------------------------ the switch
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_processors_follow_the_process_wide_switch(model, monkeypatch):
    """a differentiable=True Train processor under set_attention_backward("key_major"): the key-major kernels run, and the
    gradients stay within the bound of tests/test_hip_processors_grad.py"""
    import test_hip_processors_grad as PG
    from vorta_amd import ops, routed
    calls = []
    stock = ops.attn_bwd_key_major
    monkeypatch.setattr(ops, "attn_bwd_key_major", lambda *a, **kw: (calls.append(1), stock(*a, **kw))[1])
    monkeypatch.setattr(ops, "attn_bwd", lambda *a, **kw: pytest.fail("the query-major kernel ran under key_major"))
    monkeypatch.setattr(PG, "RATIOS", {})  # (that module's accuracy summary keeps to its own cases)
    before = routed._attention_backward
    try:
        routed.set_attention_backward("key_major")
        assert routed.attention_backward() == "key_major"
        if model == "hunyuan":
            PG.test_hunyuan_processor_gradients("train", True, torch.bfloat16)
        else:
            PG.test_wan_processor_gradients("train", torch.float16)
    finally:
        routed._attention_backward = before
    assert len(calls) == (4 if model == "hunyuan" else 3)  # one per recorded launch


def test_accuracy_summary_written():
    """max / median of e_hip / e_torch per quantity and dtype over this module's random launches and statistics cases (runs
    after them; profiles/attn_bwd_key_major_accuracy.txt comes from here when VORTA_BWD_KEY_MAJOR_ACCURACY_OUT names a file)"""
    if not RATIOS:
        return  # (selected on its own: nothing to summarise)
    lines = [f"{dt} {name}: cases {len(r)} max {max(r):.3f} median {float(np.median(r)):.3f}"
             for (dt, name), r in sorted(RATIOS.items())]
    print("\n".join(lines))
    path = os.environ.get("VORTA_BWD_KEY_MAJOR_ACCURACY_OUT")
    if path:
        with open(path, "w") as f:
            f.write("e_hip / e_torch of the key-major backward over the random launches and the statistics cases of "
                    "tests/test_hip_attention_bwd_key_major.py (bound: 2)\n" + "\n".join(lines) + "\n")
    assert all(max(r) <= 2.0 for r in RATIOS.values())
