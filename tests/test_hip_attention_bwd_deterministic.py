"""GPU: the deterministic attention backward (vorta_attn_bwd_stats + vorta_attn_bwd_dq + vorta_attn_bwd_dkv) -- the accuracy
rule of tests/test_hip_attention_bwd.py against torch autograd in float64 on the plain restatement of tests/_attn_restate.py,

    e_hip <= 2 e_torch per gradient, with e_torch the error of torch's own 16-bit autograd on the same restatement, and a
    gradient whose float64 norm is exactly zero must be exactly zero,

and what the mode is for: the same bits on every run.  Equality over repeats shows that property and cannot prove it; the proof
is structural (no atomic in either kernel, one writer per row and launch, stream order between launches), and
the precondition it rests on -- distinct rows within a key list, distinct heads in a head list -- is checked here on the
tables the package builds.

Measured on an MI355X (profiles/attn_bwd_deterministic_accuracy.txt): e_hip / e_torch 0.35-0.41 in the median and at most 0.77
for dq / dk / dv over the random launches."""
import os

import numpy as np
import pytest
import torch

import _random_launch as RL
import test_hip_attention_bwd as B
import test_hip_attention_bwd_key_major as KM
from _attn_restate import named_rows
from _util import dev

pytestmark = pytest.mark.gpu

RATIOS = {}  # (dtype name, gradient) -> list of e_hip / e_torch over the random launches
REPEATS = 5
_RANDOM = {}  # seed -> the case of a random launch that test_agrees_with_query_major looks at again


def _deterministic(q, k, v, out, d_o, bufs, w, kw, stats=None):
    from vorta_amd import ops
    if stats is None:
        stats = ops.attn_bwd_stats(q, k, v, out, d_o, do_scale=w, **kw)
    ops.attn_bwd_dq(q, k, v, out, d_o, bufs[0], stats, do_scale=w, **kw)
    ops.attn_bwd_dkv(q, k, v, out, d_o, bufs[1], bufs[2], stats, do_scale=w, **kw)
    return stats


def _check_launch(kw, shape, dtype, seed, weight, what, ratios=None):
    """one launch through the three passes: the bound, exact zeros where the launch names nothing, the "added to" contract,
    and each pass keeping to its own buffers"""
    from vorta_amd import ops
    q, k, v, d_o, w = KM._inputs(shape, dtype, seed, weight)
    out = torch.full(shape, RL.SENTINEL, dtype=dtype, device=dev())
    ops.attn_fwd(q, k, v, out, **kw)
    ref, t16 = KM._references(kw, q, k, v, d_o, w, dtype)
    zero = [torch.zeros(shape, dtype=torch.float32, device=dev()) for _ in range(3)]
    stats = _deterministic(q, k, v, out, d_o, zero, w, kw)
    sent = [torch.full(shape, 3.0, dtype=torch.float32, device=dev()) for _ in range(3)]
    ops.attn_bwd_dq(q, k, v, out, d_o, sent[0], stats, do_scale=w, **kw)
    assert (sent[1] == 3.0).all() and (sent[2] == 3.0).all(), f"{what}: the dQ pass touched dk / dv"
    dq_after = sent[0].clone()
    ops.attn_bwd_dkv(q, k, v, out, d_o, sent[1], sent[2], stats, do_scale=w, **kw)
    assert torch.equal(sent[0], dq_after), f"{what}: the dK / dV pass touched dq"
    qm, km = named_rows(kw, shape)
    for name, got, s, t, r in zip(("dq", "dk", "dv"), zero, sent, t16, ref):
        untouched = ~(qm if name == "dq" else km).to(dev())
        assert not r[untouched].any()  # (the restatement agrees on which rows those are)
        assert not got[untouched].any(), f"{what}: {name} wrote rows the launch does not name"
        assert (s[untouched] == 3.0).all(), f"{what}: {name} disturbed the sentinel of unnamed rows"
        # float32 at magnitude 3: half an ulp, 1.2e-7, per addition -- one per launch and key list that names the row
        assert torch.allclose(s, got + 3.0, rtol=1e-5, atol=1e-5), f"{what}: {name} is not sentinel + gradient"
        e = B._bound(name, got, t, r, what)
        if ratios is not None and e is not None and e[1] > 0:
            ratios.setdefault((KM._name(dtype), name), []).append(e[0] / e[1])
    return dict(q=q, k=k, v=v, d_o=d_o, w=w, out=out, ref=ref, got=zero)


# ---------------------------------------------------------------------------------------------------- named small shapes
@pytest.mark.parametrize("case", KM.NAMED)
def test_named_small_shapes(case):
    """the shapes of tests/test_hip_attention_bwd_key_major.py: they sit on the same tile edges (256-key blocks, 32-row slices,
    128-row query blocks)"""
    H, S, kw = KM._named_shapes()[case]
    for i, dtype in enumerate((torch.bfloat16, torch.float16)):
        _check_launch(kw, (H, S, 128), dtype, 50 + i, True, f"{case} {KM._name(dtype)}")


# ------------------------------------------------------------------------------------------------------- random launches
@pytest.mark.parametrize("seed", range(B.N_RANDOM))
def test_random_launch_gradients(seed):
    rng = np.random.default_rng(1000 + seed)
    dtype = (torch.bfloat16, torch.float16)[seed % 2]
    L = RL.draw(rng, device_lengths=True, heads_dev=True)
    kw = RL.kwargs(L, dev())
    case = _check_launch(kw, (L.H_buf, L.S, 128), dtype, seed, seed % 4 < 2, f"seed {seed} {RL.describe(L)}", RATIOS)
    if seed < 6:
        _RANDOM[seed] = dict(case, kw=kw)


# ------------------------------------------------------------------------------------------- agreement with query_major
@pytest.mark.parametrize("seed", range(6))
def test_agrees_with_query_major(seed):
    """the rule of test_key_major_agrees_with_query_major: the two algorithms differ by no more than the sum of their errors
    against float64, per gradient (the launch, its inputs, the float64 reference and the deterministic gradients are those of
    the random-launch test of the same seed when it has run)"""
    from vorta_amd import ops
    if seed not in _RANDOM:
        test_random_launch_gradients(seed)
    c = _RANDOM[seed]
    qm = [torch.zeros_like(x) for x in c["got"]]
    ops.attn_bwd(c["q"], c["k"], c["v"], c["out"], c["d_o"], *qm, do_scale=c["w"], **c["kw"])
    for name, a, b, r in zip(("dq", "dk", "dv"), c["got"], qm, c["ref"]):
        apart, e_a, e_b = B._fro(a.double() - b.double()), B._fro(a.double() - r), B._fro(b.double() - r)
        print(f"seed {seed} {name}: apart {apart:.3e} e_deterministic {e_a:.3e} e_query_major {e_b:.3e}")
        assert apart <= e_a + e_b, f"seed {seed} {name}: the algorithms are {apart:.3e} apart, errors {e_a:.3e} + {e_b:.3e}"


# ----------------------------------------------------------------------------------------------------- bit-reproducibility
def _repro_cases():
    # in each of them the two atomic algorithms have many concurrent adders per row
    return {
        # key-major would have 8 key blocks adding into every dq row, query-major 16 query blocks into every dk row
        "dense": (4, 2048, dict(n_q=2048, n_kv=2048)),
        # two groups of 300 queries; key lists of 1100 rows that share the rows 300..1099 of the first (5 key blocks each)
        "overlapping_lists": (2, 1408, dict(n_q=600, q_group_len=300, n_kv=1100, kv_rows=KM._two_lists(1100, shift=300),
                                            kv_rows_stride_g=1100)),
    }


@pytest.mark.parametrize("case", ["dense", "overlapping_lists"])
def test_same_bits_on_every_run(case):
    from vorta_amd import ops
    H, S, kw = _repro_cases()[case]
    shape = (H, S, 128)
    q, k, v, d_o, w = KM._inputs(shape, torch.bfloat16, 11, True)
    out = torch.empty_like(q)
    ops.attn_fwd(q, k, v, out, **kw)
    first = None
    for rep in range(REPEATS):
        bufs = [torch.zeros(shape, dtype=torch.float32, device=dev()) for _ in range(3)]
        _deterministic(q, k, v, out, d_o, bufs, w, kw)
        assert all(b.any() for b in bufs)
        if first is None:
            first = bufs
        for name, a, b in zip(("dq", "dk", "dv"), first, bufs):
            assert torch.equal(a, b), f"{case}: {name} of run {rep} differs from run 0"


@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_soft_mixture_same_bits_on_every_run(model, golden):
    from vorta_amd.routed import soft_mixture_attention_autograd
    geom, t, te, q, k, v, sc, G = B._mixture_case(model, torch.bfloat16, golden)
    first = None
    for rep in range(REPEATS):
        leaves = [x.clone().requires_grad_(True) for x in (q, k, v, sc)]
        out = soft_mixture_attention_autograd(*leaves, geom, backward="deterministic", model=model, text_len=t, text_valid=te)
        (out * G).sum().backward()
        grads = [x.grad for x in leaves]
        assert all(g.any() for g in grads)
        if first is None:
            first = grads
        for name, a, b in zip(("dq", "dk", "dv", "dscores"), first, grads):
            assert torch.equal(a, b), f"{model}: {name} of backward {rep} differs from backward 0"


# ------------------------------------------------------------------- the precondition, on the tables the package builds
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_recorded_key_lists_and_head_lists_are_distinct(model, golden):
    """vorta_attn_bwd_dkv's one-writer-per-row rests on it: the first n_kv rows of every key list are distinct, and a
    head_list names distinct heads (a host-side check of what routed_attention records)"""
    from vorta_amd.routed import HeadRouting, routed_attention
    geom, t, te, q, k, v, sc, G = B._mixture_case(model, torch.bfloat16, golden)
    bufs, launches = [torch.empty_like(q) for _ in range(3)], []
    routed_attention(q, k, v, HeadRouting.every_head_everywhere(q.shape[1], q.device), geom, expert_outs=bufs, fp8=False,
                     record=launches, model=model, text_len=t, text_valid=te)
    assert len(launches) == (4 if model == "hunyuan" else 3)
    seen_lists = seen_heads = 0
    for c in launches:
        n_kv = c["n_kv"]
        if c.get("kv_rows") is not None:
            rows, sg = c["kv_rows"].cpu(), c.get("kv_rows_stride_g", 0)
            if sg > 0:
                n_lists = c["n_key_lists"] if c.get("q_block_table") is not None else -(-c["n_q"] // (c.get("q_group_len") or c["n_q"]))
                flat = rows.reshape(-1)
                lists = [flat[g * sg: g * sg + n_kv] for g in range(n_lists)]
            else:
                lists = [r[:n_kv] for r in (rows if rows.dim() == 2 else rows[None])]
            for i, lst in enumerate(lists):
                assert lst.numel() == n_kv and torch.unique(lst).numel() == n_kv, f"{model}: key list {i} repeats a row"
            seen_lists += len(lists)
        if c.get("head_list") is not None:
            heads = c["head_list"].cpu()[: c["n_heads"]] if c.get("n_heads") is not None else c["head_list"].cpu()
            assert torch.unique(heads).numel() == heads.numel(), f"{model}: a head_list names a head twice"
            seen_heads += 1
    assert seen_lists > 0  # (the coreset keep lists and the sliding-tile tables)
    print(f"{model}: {seen_lists} key lists and {seen_heads} head lists checked")


# ------------------------------------------------------------------------------------------------ soft mixture, end to end
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_soft_mixture_autograd_deterministic(model, dtype, golden):
    from vorta_amd.routed import HeadRouting, routed_attention, soft_mixture_attention_autograd
    geom, t, te, q, k, v, sc, G = B._mixture_case(model, dtype, golden)
    H = q.shape[1]
    kwm = dict(model=model, text_len=t, text_valid=te)
    with torch.no_grad():
        by_query = soft_mixture_attention_autograd(q, k, v, sc, geom, backward="query_major", **kwm)
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v, sc)]
    out = soft_mixture_attention_autograd(*leaves, geom, backward="deterministic", **kwm)
    assert torch.equal(out, by_query)  # the forward does not depend on the backward's algorithm
    (out * G).sum().backward()
    dq, dk, dv, dsc = (x.grad for x in leaves)
    bufs, launches = [torch.empty_like(q) for _ in range(3)], []
    routed_attention(q, k, v, HeadRouting.every_head_everywhere(H, q.device), geom, expert_outs=bufs, fp8=False,
                     record=launches, **kwm)
    bufs3 = [b[0] for b in bufs]
    want = torch.stack([(G[0].double() * b.double()).sum((1, 2)) for b in bufs3], dim=1)
    t16 = torch.stack([(G[0] * b).sum((1, 2)) for b in bufs3], dim=1)
    B._bound("dscores", dsc[0], t16, want, f"deterministic {model} {dtype}")
    ref, _ = B._mixture_reference(launches, bufs3, q, k, v, sc, G, torch.float64)
    y16, _ = B._mixture_reference(launches, bufs3, q, k, v, sc, G, dtype)
    for name, got, a, b in zip(("dq", "dk", "dv"), (dq, dk, dv), y16, ref):
        assert got.dtype == dtype and got.shape == q.shape
        B._bound(name, got[0], a, b, f"deterministic {model} {dtype}")
    if t > te:  # padded text rows take no gradient
        for g in (dq, dk, dv):
            assert not g[:, :, B.S_VID + te:].any()


def test_dense_attention_autograd_deterministic():
    from vorta_amd.routed import dense_attention, dense_attention_autograd
    gen = torch.Generator(device="cpu").manual_seed(3)
    for dtype in (torch.bfloat16, torch.float16):
        q = torch.randn((1, 3, 200, 128), generator=gen).to(dtype).to(dev())
        k, v = (torch.randn((1, 3, 333, 128), generator=gen).to(dtype).to(dev()) for _ in range(2))
        G = torch.randn(q.shape, generator=gen).to(dtype).to(dev())
        leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
        out = dense_attention_autograd(*leaves, kv_valid=300, q_valid=190, backward="deterministic")
        assert torch.equal(out, dense_attention(q, k, v, kv_valid=300, q_valid=190))
        (out * G).sum().backward()

        def grads(dt):
            x = [a[0].detach().to(dt).requires_grad_(True) for a in (q, k, v)]
            p = torch.softmax(x[0] @ x[1][:, :300].transpose(1, 2) / 128 ** 0.5, dim=-1) @ x[2][:, :300]
            p = torch.cat([p[:, :190], torch.zeros_like(p[:, 190:])], dim=1)
            return torch.autograd.grad(p, x, G[0].to(dt))

        for name, got, a, b in zip(("dq", "dk", "dv"), leaves, grads(dtype), grads(torch.float64)):
            B._bound(name, got.grad[0], a, b, f"deterministic dense {dtype}")
        assert not leaves[0].grad[:, :, 190:].any() and not leaves[1].grad[:, :, 300:].any()


# ------------------------------------------------------------------------------------------------------------ the switch
@pytest.mark.parametrize("model", ["hunyuan", "wan"])
def test_processors_follow_the_process_wide_switch(model, monkeypatch):
    """a differentiable=True Train processor under set_attention_backward("deterministic"): only the three deterministic
    passes run, and the gradients stay within the bound of tests/test_hip_processors_grad.py"""
    import test_hip_processors_grad as PG
    from vorta_amd import ops, routed
    calls = []
    stock = ops.attn_bwd_dkv
    monkeypatch.setattr(ops, "attn_bwd_dkv", lambda *a, **kw: (calls.append(1), stock(*a, **kw))[1])
    monkeypatch.setattr(ops, "attn_bwd", lambda *a, **kw: pytest.fail("the query-major kernel ran under deterministic"))
    monkeypatch.setattr(ops, "attn_bwd_key_major", lambda *a, **kw: pytest.fail("the key-major kernel ran under deterministic"))
    monkeypatch.setattr(PG, "RATIOS", {})  # (that module's accuracy summary keeps to its own cases)
    before = routed._attention_backward
    try:
        routed.set_attention_backward("deterministic")
        assert routed.attention_backward() == "deterministic"
        if model == "hunyuan":
            PG.test_hunyuan_processor_gradients("train", True, torch.bfloat16)
        else:
            PG.test_wan_processor_gradients("train", torch.float16)
    finally:
        routed._attention_backward = before
    assert len(calls) == (4 if model == "hunyuan" else 3)  # one per recorded launch


def test_accuracy_summary_written():
    """max / median of e_hip / e_torch per gradient and dtype over this module's random launches (runs after them;
    profiles/attn_bwd_deterministic_accuracy.txt comes from here when VORTA_BWD_DETERMINISTIC_ACCURACY_OUT names a file)"""
    if not RATIOS:
        return  # (selected on its own: nothing to summarise)
    lines = [f"{dt} {name}: cases {len(r)} max {max(r):.3f} median {float(np.median(r)):.3f}"
             for (dt, name), r in sorted(RATIOS.items())]
    print("\n".join(lines))
    path = os.environ.get("VORTA_BWD_DETERMINISTIC_ACCURACY_OUT")
    if path:
        with open(path, "w") as f:
            f.write("e_hip / e_torch of the deterministic backward over the random launches of "
                    "tests/test_hip_attention_bwd_deterministic.py (bound: 2)\n" + "\n".join(lines) + "\n")
    assert all(max(r) <= 2.0 for r in RATIOS.values())
