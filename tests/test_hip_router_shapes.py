"""vorta_router_route / vorta_route_plan / vorta_route_scores at the shapes the real models use and at the edges of their
loops, against the rounding model of tests/_side_kernel_models.py (float64 with the kernel's roundings by design, a derived
bound per logit and per score).  The router entry points are called through vorta_amd._C.RouterArgs as ops.router_route calls
them, so that the test owns ws_logits and can read the logits: that part is white-box by intent, the score checks are the
contract."""
import ctypes as C

import numpy as np
import pytest
import torch

import _side_kernel_models as M
from oracle import vorta_oracle as O
from _util import dev

pytestmark = pytest.mark.gpu

CASES = sorted(M.ROUTER_CASES)
FIGURES = {}  # case -> dict(logit, score, unclear)


def _route(temb, W, b, H, tau, layers=None, out=None):
    """the ABI as ops.router_route / ops.route_plan call it; returns (scores, expert, lists, counts, logits) on the device, with
    a leading layer axis when `layers` is given"""
    from vorta_amd import _C, ops
    B, E = temb.shape
    L = layers or 1
    lead = () if layers is None else (L,)
    if out is None:
        out = (torch.empty(lead + (B, H, 3), dtype=temb.dtype, device=dev()),
               torch.full(lead + (H,), -7, dtype=torch.int32, device=dev()),
               torch.full(lead + (3, H), -7, dtype=torch.int32, device=dev()),
               torch.full(lead + (3,), -7, dtype=torch.int32, device=dev()),
               torch.full(lead + (B, H, 3), float("nan"), dtype=torch.float32, device=dev()))
    scores, expert, lists, counts, ws = out
    a = _C.RouterArgs()
    a.struct_size = C.sizeof(_C.RouterArgs)
    a.dtype = ops._DT[temb.dtype]
    a.batch, a.embed_dim, a.heads, a.n_experts = B, E, H, 3
    a.temb, a.weight, a.bias = temb.data_ptr(), W.data_ptr(), b.data_ptr()
    a.tau = tau
    a.scores, a.expert_of_head = scores.data_ptr(), expert.data_ptr()
    a.head_lists, a.head_counts, a.ws_logits = lists.data_ptr(), counts.data_ptr(), ws.data_ptr()
    if layers is None:
        _C.check(_C.lib().vorta_router_route(C.byref(a), ops._stream()), "vorta_router_route")
    else:
        _C.check(_C.lib().vorta_route_plan(C.byref(a), L, ops._stream()), "vorta_route_plan")
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def _check_lists(expert, lists, counts, H):
    """head_lists[e][:counts[e]] are the ascending heads of expert e; the counts sum to H"""
    for e in range(lists.shape[0]):
        assert np.array_equal(lists[e, : counts[e]], np.nonzero(expert == e)[0]), e
    assert counts.sum() == H and ((expert >= 0) & (expert < lists.shape[0])).all()


@pytest.mark.parametrize("case", CASES)
def test_router_case(case):
    dtype, B, E, H = M.ROUTER_CASES[case]
    temb, W, b = M.router_inputs(case)
    m = M.router_model(temb, W, b, H, dtype)
    d = [t.to(dev()) for t in (temb, W, b)]
    fig = FIGURES.setdefault(case, dict(logit=0.0, score=0.0, unclear={}))
    for tau in M.ROUTER_TAUS:
        scores, expert, lists, counts, ws = (t.cpu() for t in _route(*d, H, tau))
        lg, sc = ws.double().numpy(), scores.double().numpy()
        assert np.isfinite(lg).all() and np.isfinite(sc).all()
        rl = np.abs(lg - m.logit64) / m.logit_bound(lg)
        rs = np.abs(sc - m.scores64) / m.score_bound(lg)
        clear = m.clear_heads(tau)
        fig["logit"], fig["score"] = max(fig["logit"], float(rl.max())), max(fig["score"], float(rs.max()))
        fig["unclear"][tau] = int((~clear).sum())
        print(f"router {case} tau {tau}: worst logit error / lb {rl.max():.3f}, score error / sb {rs.max():.3f}, "
              f"{(~clear).sum()} of {H} heads unclear")
        assert rl.max() <= 1, np.argwhere(rl > 1)[:8]
        assert rs.max() <= 1, np.argwhere(rs > 1)[:8]
        # the rule, applied exactly to the scores the kernel returned, with tau rounded to T (torch's comparison of a tensor
        # of dtype T with a Python scalar, hunyuan.py:623)
        expert = expert.numpy()
        want = O.route_heads(sc, float(torch.tensor(tau, dtype=dtype)))
        assert np.array_equal(expert, want)
        _check_lists(expert, lists.numpy(), counts.numpy(), H)
        assert np.array_equal(expert[clear], m.route64(tau)[clear])


def test_silu_of_large_arguments():
    """temb = -120 everywhere: silu(-120) = -120 / (1 + inf) must be zero, not NaN, so the logits are the bias alone; +120 is
    passed through unchanged (case d plants +-120, +-20 and 0 among random values as well)"""
    dtype, H, E = torch.float16, 2, 16
    W = torch.full((3 * H, E), 2.0, dtype=dtype)
    b = torch.tensor([0.5, -1.0, 2.0, 0.0, 0.25, -3.0], dtype=dtype)
    for v, dot in ((-120.0, 0.0), (120.0, 120.0 * 2 * E)):
        temb = torch.full((1, E), v, dtype=dtype)
        scores, _, _, _, ws = _route(temb.to(dev()), W.to(dev()), b.to(dev()), H, 0.0)
        want = (b.double() + dot).to(dtype).float().view(1, H, 3)
        assert torch.equal(ws.cpu(), want), (v, ws)
        assert torch.isfinite(scores.float()).all()
    planted = M.router_inputs(M.PLANTED_CASE)[0][0, 1:1 + len(M.PLANTED)]
    assert planted.tolist() == list(M.PLANTED)


def test_router_refuses_more_than_1024_heads():
    dtype = torch.bfloat16
    temb = torch.zeros((1, 8), dtype=dtype, device=dev())
    W = torch.zeros((3 * 1025, 8), dtype=dtype, device=dev())
    b = torch.zeros(3 * 1025, dtype=dtype, device=dev())
    with pytest.raises(ValueError):
        _route(temb, W, b, 1025, 0.5)
    from vorta_amd import ops
    with pytest.raises(ValueError):
        ops.route_scores(torch.zeros((1, 1025, 3), dtype=dtype, device=dev()), 0.5)


@pytest.mark.parametrize("case,layers", [("a", 3), ("f", 3), ("a", 1)])
def test_route_plan_equals_router_route_per_layer(case, layers):
    """every layer of one vorta_route_plan launch (blockIdx.y = layer) against vorta_router_route on that layer's slice of the
    weights and biases, bit for bit: scores, experts, lists, counts and logits; a second call into the same buffers writes
    the same"""
    from vorta_amd import ops
    dtype, B, E, H = M.ROUTER_CASES[case]
    temb, W, b = (t.to(dev()) for t in M.router_inputs(case, layers=layers))
    tau = 0.5
    plan = _route(temb, W, b, H, tau, layers=layers)
    for l in range(layers):
        one = _route(temb, W[l].contiguous(), b[l].contiguous(), H, tau)
        n = one[3].cpu()
        for name, p, o in zip(("scores", "expert", "lists", "counts", "logits"), plan, one):
            if name == "lists":  # entries past counts[e] are not written by either
                for e in range(3):
                    assert torch.equal(p[l][e, : n[e]], o[e, : n[e]]), (l, e)
            else:
                assert torch.equal(_bits(p[l]), _bits(o)), (name, l)
    if layers > 1:
        assert not torch.equal(plan[1][0], plan[1][1]) or not torch.equal(plan[1][1], plan[1][2])  # the layers do differ
    # ops.route_plan with out= : the same buffers, the same contents
    first = ops.route_plan(temb, W, b, H, tau)
    for p, f in zip(plan[:2] + plan[3:4], first[:2] + first[3:4]):
        assert torch.equal(p, f)
    keep = [t.clone() for t in first]
    ptrs = [t.data_ptr() for t in first]
    for t in first:
        t.fill_(-1 if t.dtype == torch.int32 else 0.25)
    again = ops.route_plan(temb, W, b, H, tau, out=first)
    torch.cuda.synchronize()
    assert [t.data_ptr() for t in again] == ptrs
    n = keep[3].cpu()
    for i, (x, y) in enumerate(zip(again, keep)):
        if i == 2:
            for l in range(layers):
                for e in range(3):
                    assert torch.equal(x[l, e, : n[l, e]], y[l, e, : n[l, e]])
        else:
            assert torch.equal(x, y), i


# ------------------------------------------------------------------------------------------------ route_scores
SCORE_DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _cpu_rule(scores, tau):
    """expert per head as the reference computes it (hunyuan.py:620-624), by torch on the CPU in the scores' dtype: top-1 of
    batch item 0 (first maximum), expert 0 where `top < tau`"""
    s = scores[0].cpu()
    top = s.max(-1).values
    first = (s == top[:, None]).int().argmax(-1)  # first maximal index
    return torch.where(top < tau, torch.zeros_like(first), first).int().numpy()


def _run_scores(scores, tau):
    from vorta_amd import ops
    expert, lists, counts = ops.route_scores(scores.to(dev()), tau)
    torch.cuda.synchronize()
    expert, lists, counts = expert.cpu().numpy(), lists.cpu().numpy(), counts.cpu().numpy()
    _check_lists(expert, lists, counts, scores.shape[1])
    return expert, counts


@pytest.mark.parametrize("H", [1, 64, 65, 1024])
@pytest.mark.parametrize("dtype", SCORE_DTYPES, ids=M.dtype_name)
def test_route_scores_heads_ties_and_batch(dtype, H):
    """random scores with exact two-way and three-way ties (the first expert wins) and a batch item 1 that alone would route
    every head differently"""
    g = torch.Generator().manual_seed(H)
    s0 = torch.softmax(2 * torch.randn((H, 3), generator=g), -1).to(dtype)
    for h in range(0, H, 5):  # two-way ties for the top score, at every pair of positions
        i, j = [(0, 1), (0, 2), (1, 2)][(h // 5) % 3]
        s0[h, i] = s0[h, j] = s0[h].max()
    for h in range(3, H, 7):  # three-way ties
        s0[h] = s0[h, 0]
    s1 = s0.roll(1, dims=-1).clone()
    tau = 0.2
    want = _cpu_rule(s0[None], tau)
    other = _cpu_rule(s1[None], tau)
    for h in range(H):  # item 1 would send every head elsewhere
        if other[h] == want[h]:
            s1[h] = torch.eye(3)[(int(want[h]) + 1) % 3].to(dtype)
    assert (_cpu_rule(s1[None], tau) != want).all()
    expert, counts = _run_scores(torch.stack([s0, s1]), tau)
    assert np.array_equal(expert, want)
    for h in range(H):  # and written out per head: the FIRST maximal expert, or expert 0 below tau
        row = s0[h].tolist()
        assert expert[h] == (row.index(max(row)) if max(row) >= float(torch.tensor(tau, dtype=dtype)) else 0), (h, row)
    # every head below tau: all to expert 0, counts (H, 0, 0)
    low = torch.softmax(0.1 * torch.randn((2, H, 3), generator=g), -1).to(dtype)
    expert, counts = _run_scores(low, 0.75)
    assert not expert.any() and counts.tolist() == [H, 0, 0]


@pytest.mark.parametrize("dtype", SCORE_DTYPES, ids=M.dtype_name)
def test_route_scores_rounds_tau_to_the_score_dtype(dtype):
    """tau values that T does not represent, one above and one below its rounded value, against top scores equal to round_T(tau)
    and one ulp on either side: the expectation is `scores_T[0].max(-1).values < tau` evaluated by torch on the CPU in dtype T
    (hunyuan.py:623) -- a kernel comparing with the unrounded tau gets the middle head wrong for one of the two"""
    for base in (0.4, 0.5, 0.9):  # (above 1/3: the other two experts share the rest and stay below)
        t = torch.tensor(base, dtype=dtype)
        up, down = torch.nextafter(t, torch.tensor(2.0, dtype=dtype)), torch.nextafter(t, torch.tensor(0.0, dtype=dtype))
        ulp = float(up.double() - t.double())
        for tau in (float(t.double()) + 0.3 * ulp, float(t.double()) - 0.2 * ulp):
            assert float(torch.tensor(tau, dtype=dtype).double()) == float(t.double()) and tau != float(t.double())
            tops = torch.stack([down, t, up])
            rest = ((1 - tops.double()) / 2).to(dtype)
            s0 = torch.stack([rest, tops, rest], -1)  # the top score sits at expert 1
            s1 = torch.stack([tops, rest, rest], -1)
            want = ((s0.max(-1).values < tau).int() ^ 1).numpy()  # torch: tensor of dtype T < Python scalar
            assert want.tolist() == [0, 1, 1]
            expert, _ = _run_scores(torch.stack([s0, s1]), tau)
            assert np.array_equal(expert, want), (dtype, tau, expert)


def test_accuracy_summary_written():
    """worst error / bound per router case (runs after them; the router section of profiles/side_kernels_accuracy.txt comes from
    here when VORTA_SIDE_KERNELS_ACCURACY_OUT names a file)"""
    if not FIGURES:
        return  # (selected on its own: nothing to summarise)
    lines = []
    for case, f in sorted(FIGURES.items()):
        dtype, B, E, H = M.ROUTER_CASES[case]
        unclear = ", ".join(f"tau {t}: {n}" for t, n in f["unclear"].items())
        lines.append(f"router {case} {M.dtype_name(dtype)} batch {B} E {E} H {H}: logit error / lb {f['logit']:.4f}  "
                     f"score error / sb {f['score']:.4f}  unclear heads ({unclear}) cap {M.unclear_cap(H)}")
    M.write_record_section("router (tests/test_hip_router_shapes.py)", lines)
    assert all(f["logit"] <= 1 and f["score"] <= 1 for f in FIGURES.values())
