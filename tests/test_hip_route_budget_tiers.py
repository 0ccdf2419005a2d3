"""GPU: `ops.route_budget_tiers` (vorta_route_budget_tiers) against the host rule, `vorta.patch.routes_within_cost_share`, which
is the definition.  The host rule is evaluated on CPU copies of the records; the expert table, the tier table, the counts,
every list up to its count, the cost share and the level must be EQUAL -- no tolerance: rel is two correctly rounded float32
operations, a cost a chain of double products and sums from integer counts, the same chain on both sides.

Crafted records (the rows of tests/test_hip_route_fidelity_tiers.py: ties across and within tiers, NaN, inf, sq_ref == 0, no
exact tier); random records with errors from its small sets, so that ties are common, at H in {1, 5, 24, 40, 257, 1024} -- 257
runs the strided loop past 256 lanes, 1024 is the limit -- x 1..3 tiers in every order; shares that meet a budget exactly; the
sentinel past a count; a graph replay on new records; the error codes; the operator.  Every case is one launch of one
workgroup."""
import ctypes as C

import pytest
import torch

from _util import dev
from test_hip_route_fidelity_tiers import (COSTS, CRAFTED, CRAFTED_I8, CRAFTED_NAT, CRAFTED_REF, TIER_ORDERS, WORKS, _fid, _fids,
                                           _record)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
# 0.5, 0.75, 0.25 and 1.0 meet budgets exactly wherever the costs are binary fractions (COSTS[1:4] with the small works)
SHARES = [0.05, 0.25, 1 / 3, 0.4, 0.5, 0.59, 0.75, 0.9, 1.0, 2.0]


def _host(tiers, sq_ref, sq_errs, work, share, cost):
    from vorta_amd.patch import routes_within_cost_share
    r = routes_within_cost_share(_fids(tiers, sq_ref.cpu(), [e.cpu() for e in sq_errs]), share, dict(work=work), tier_cost=cost)
    # the device speaks the caller's tier INDEX
    return r.experts.tolist(), [list(tiers).index(t) for t in r.tiers.tolist()], float(r.level), float(r.cost_share)


def _run(fids, share, work, cost):
    from vorta_amd import ops
    return ops.route_budget_tiers(fids, max_cost_share=share, work=work, tier_cost=cost, cost_share=True)


def _to_host(got):
    return [t.cpu().tolist() for t in got[:4]] + [float(got[4]), float(got[5])]


def _check(got, want, case):
    """one call's device outputs (already on the host) against the host rule's"""
    expert, tier, lists, counts, level, share = got
    want_expert, want_tier, want_level, want_share = want
    H, T = len(want_expert), len(counts)
    assert expert == want_expert, f"{case}: expert table {expert} != host {want_expert}"
    assert tier == want_tier, f"{case}: tier table {tier} != host {want_tier}"
    for t in range(T):
        for e in range(3):
            heads = [h for h in range(H) if want_tier[h] == t and want_expert[h] == e]
            assert counts[t][e] == len(heads), f"{case}: count of tier index {t} expert {e}: {counts}"
            assert lists[t][e][:len(heads)] == heads, f"{case}: list of tier index {t} expert {e}"
    assert level == want_level, f"{case}: level {level} != host {want_level}"
    assert share == want_share, f"{case}: cost share {share} != host {want_share}"


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("work", WORKS[:4])
def test_crafted_records(work, cost):
    cases, outs = [], []
    for n in (1, 2, 3):
        for tiers in TIER_ORDERS[n]:
            errs = [torch.tensor(CRAFTED[t]) for t in tiers]
            ref = torch.tensor(CRAFTED_REF)
            for share in (0.25, 0.5, 0.75, 1.0):
                got = _run(_fids(tiers, ref, errs, dev()), share, work, cost)
                assert all(t.is_cuda for t in got) and [t.dtype for t in got] == [torch.int32] * 4 + [torch.float32] * 2
                cases.append((tiers, ref, errs, work, share, cost))
                outs.append(got)
    torch.cuda.synchronize()
    for case, got in zip(cases, outs):
        _check(_to_host(got), _host(*case), f"crafted tiers={case[0]} share={case[4]} work={work} cost={cost}")


def test_the_worked_examples_by_hand():
    k2 = lambda *ks: [NAN if k is None else k * k / 4096.0 for k in ks]  # noqa: E731  (rel = k / 64, exactly)
    fids = {"i8pv": _fid([1.0, 1.0], [k2(3, 7, 1), k2(5, 14, 1)], dev()), "native": _fid([1.0, 1.0], [k2(2, 6, None), k2(4, 12, None)], dev())}
    half = {"i8pv": 0.5, "native": 1.0}
    expert, tier, lists, counts, level, share = _to_host(_run(fids, 0.5, (3.0, 2.0, 1.0), half))
    assert (expert, tier, level, share) == ([0, 0], [0, 0], 1 / 64, 0.5) and counts == [[2, 0, 0], [0, 0, 0]]
    expert, tier, lists, counts, level, share = _to_host(_run(fids, 0.4, (3.0, 2.0, 1.0), half))
    assert (expert, tier, level) == ([1, 1], [0, 0], 5 / 64) and share == float(torch.tensor(1 / 3, dtype=torch.float32))
    assert lists[0][1] == [0, 1]
    # ties at one rel: the lowest heads move first, a budget met with equality is met; an equal cost moves no head
    four = {"native": _fid([1.0] * 4, [k2(4, 63, None)] * 4, dev())}
    assert _to_host(_run(four, 0.75, (4.0, 2.0, 1.0), None))[0] == [1, 1, 0, 0]
    assert _to_host(_run(four, 0.75 - 2.0 ** -20, (4.0, 2.0, 1.0), None))[0] == [1, 1, 1, 0]
    same = {"native": _fid([1.0, 1.0], [k2(1, 3, None), k2(5, 3, None)], dev())}
    got = _to_host(_run(same, 0.5, (4.0, 2.0, 2.0), None))
    assert got[0] == [1, 2] and got[4] == 3 / 64 and got[5] == 0.5
    # the candidates run out: the state of the largest level, over the budget
    out = {"i8pv": _fid([1.0, 1.0], [k2(2, 3, 1), [NAN, INF, NAN]], dev())}
    got = _to_host(_run(out, 0.5, (3.0, 2.0, 1.0), half))
    assert got[0] == [2, 0] and got[4] == 3 / 64 and got[5] > 0.5


@pytest.mark.parametrize("n_tiers", [1, 2, 3])
@pytest.mark.parametrize("H", [1, 5, 24, 40, 257, 1024])
def test_random_records_equal_the_host_rule(H, n_tiers):
    seeds = 6 if H == 1024 else 16 if H == 257 else 60
    g = torch.Generator().manual_seed(7 * H + n_tiers)
    cases, outs = [], []
    for seed in range(seeds):
        tiers, sq_ref, sq_errs, work, _, cost = _record(H, n_tiers, seed)
        share = SHARES[int(torch.randint(0, len(SHARES), (1,), generator=g))]
        cases.append((tiers, sq_ref, sq_errs, work, share, cost))
        outs.append(_run(_fids(tiers, sq_ref, sq_errs, dev()), share, work, cost))
    torch.cuda.synchronize()
    tables, levels, exact, partial = set(), set(), 0, 0
    for seed, (case, got) in enumerate(zip(cases, outs)):
        tiers, sq_ref, sq_errs, work, share, cost = case
        want = _host(*case)
        _check(_to_host(got), want, f"H={H} seed={seed} tiers={tiers} share={share} work={work} cost={cost}")
        tables.add((tuple(want[0]), tuple(want[1])))
        levels.add(want[2])
        exact += want[3] == share
    assert len(tables) >= (2 if H == 1 else 5) and len(levels) >= 2  # the draws do exercise the rule
    print(f"H={H} n_tiers={n_tiers}: {len(tables)} tables, {len(levels)} levels, {exact} budgets met exactly")


def _raw_args(ref_t, err_t, expert, tier, lists, counts, share_t, level_t, **kw):
    from vorta_amd import _C
    a = _C.RouteBudgetTiersArgs()
    a.struct_size, a.heads, a.n_tiers, a.exact_tier, a.max_cost_share = C.sizeof(a), ref_t.numel(), 2, 1, 0.5
    a.sq_ref, a.sq_err = ref_t.data_ptr(), err_t.data_ptr()
    a.expert_of_head, a.tier_of_head = expert.data_ptr(), tier.data_ptr()
    a.head_lists, a.head_counts = lists.data_ptr(), counts.data_ptr()
    a.cost_share, a.level = share_t.data_ptr(), level_t.data_ptr()
    a.work[0], a.work[1], a.work[2] = 3.0, 2.0, 1.0
    a.tier_cost[0], a.tier_cost[1], a.tier_cost[2] = 0.59, 1.0, NAN  # (the third is past n_tiers: not looked at)
    for key, value in kw.items():
        if key in ("work", "tier_cost"):
            getattr(a, key)[value[0]] = value[1]
        else:
            setattr(a, key, value)
    return a


def test_error_codes_and_nothing_is_launched_and_entries_past_a_count_keep_the_sentinel():
    from vorta_amd import _C, ops
    H = len(CRAFTED_REF)
    sq_ref = torch.tensor(CRAFTED_REF, device=dev())
    sq_err = torch.tensor([CRAFTED_I8, CRAFTED_NAT], device=dev())
    outs = [torch.full(shape, -7, dtype=torch.int32, device=dev()) for shape in ((H,), (H,), (2, 3, H), (2, 3))]
    outs += [torch.full((1,), -7.0, device=dev()) for _ in range(2)]
    lib, stream = _C.lib(), torch.cuda.current_stream().cuda_stream
    bad = [dict(heads=1025), dict(heads=0), dict(n_tiers=0), dict(n_tiers=4), dict(exact_tier=-2), dict(exact_tier=2),
           dict(sq_ref=None), dict(sq_err=None), dict(expert_of_head=None), dict(tier_of_head=None), dict(head_lists=None),
           dict(head_counts=None), dict(max_cost_share=0.0), dict(max_cost_share=-0.5), dict(max_cost_share=NAN),
           dict(work=(1, 0.0)), dict(work=(0, INF)), dict(work=(2, NAN)), dict(tier_cost=(0, 0.0)), dict(tier_cost=(1, -1.0)),
           dict(tier_cost=(1, INF)), dict(tier_cost=(0, NAN)), dict(n_tiers=3, exact_tier=1),  # (the third cost is NaN)
           dict(struct_size=C.sizeof(_C.RouteBudgetTiersArgs) - 8)]
    for kw in bad:
        assert lib.vorta_route_budget_tiers(C.byref(_raw_args(sq_ref, sq_err, *outs, **kw)), stream) == _C.VORTA_EINVAL, kw
    assert lib.vorta_route_budget_tiers(None, stream) == _C.VORTA_EINVAL
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs), "a refused call wrote its outputs"
    assert lib.vorta_sizeof(17) == -1  # (a pure addition: the block reports its size through a symbol of its own)
    assert lib.vorta_route_budget_tiers_args_size() == C.sizeof(_C.RouteBudgetTiersArgs)
    assert lib.vorta_route_budget_tiers(C.byref(_raw_args(sq_ref, sq_err, *outs)), stream) == _C.VORTA_OK  # the same block
    torch.cuda.synchronize()
    want = _host((2, 0), sq_ref, list(sq_err), (3.0, 2.0, 1.0), 0.5, {2: 0.59, 0: 1.0})
    expert, tier, lists, counts = (t.cpu().tolist() for t in outs[:4])
    assert (expert, tier, float(outs[5]), float(outs[4])) == want
    for t in range(2):
        for e in range(3):
            heads = [h for h in range(H) if want[1][h] == t and want[0][h] == e]
            assert counts[t][e] == len(heads) and lists[t][e] == heads + [-7] * (H - len(heads)), (t, e)  # past the count: not written
    assert sum(sum(c) for c in counts) == H and max(max(c) for c in counts) < H  # (some sentinel does survive)
    # the optional outputs may be left out
    a = _raw_args(sq_ref, sq_err, *outs)
    a.cost_share = a.level = None
    outs[4].fill_(-7.0), outs[5].fill_(-7.0)
    assert lib.vorta_route_budget_tiers(C.byref(a), stream) == _C.VORTA_OK
    torch.cuda.synchronize()
    assert float(outs[4]) == -7.0 and float(outs[5]) == -7.0 and outs[0].cpu().tolist() == want[0]
    fid = _fid(CRAFTED_REF, CRAFTED_I8, dev())
    big = _fid([1.0] * 1025, [[0.0, 0.0, NAN]] * 1025, dev())
    with pytest.raises(ValueError, match="vorta_route_budget_tiers"):
        ops.route_budget_tiers({"i8pv": big}, max_cost_share=0.5)
    with pytest.raises(ValueError, match="vorta_route_budget_tiers"):
        ops.route_budget_tiers({"i8pv": fid}, max_cost_share=0.5, work=(3.0, 0.0, 1.0))
    for share in (0.0, -1.0, NAN, None):
        with pytest.raises(ValueError, match="max_cost_share"):
            ops.route_budget_tiers({"i8pv": fid}, max_cost_share=share)
    with pytest.raises(ValueError, match="tier_cost"):
        ops.route_budget_tiers({"i8pv": fid}, max_cost_share=0.5, tier_cost={"i8pv": 0.0})
    with pytest.raises(ValueError, match="tier"):
        ops.route_budget_tiers({3: fid}, max_cost_share=0.5)
    with pytest.raises(ValueError, match="ONE layer"):
        ops.route_budget_tiers({"i8pv": _fid([CRAFTED_REF], [CRAFTED_I8], dev())}, max_cost_share=0.5)


def test_graph_replay_follows_the_statistics_in_the_buffers():
    H, tiers, share = 40, (2, 1, 0), 0.4
    _, sq_ref, sq_errs, work, _, cost = _record(H, 3, 0)
    static = _fids(tiers, sq_ref.to(dev()), [e.to(dev()) for e in sq_errs])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        _run(static, share, work, cost)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = _run(static, share, work, cost)
    tables = set()
    for seed in (0, 1, 2, 3):
        _, new_ref, new_errs, _, _, _ = _record(H, 3, seed)
        static[tiers[0]].sq_ref.copy_(new_ref)
        for t, e in zip(tiers, new_errs):
            static[t].sq_err.copy_(e)
        graph.replay()
        torch.cuda.synchronize()
        want = _host(tiers, new_ref, new_errs, work, share, cost)
        _check(_to_host(got), want, f"replay seed {seed}")
        tables.add((tuple(want[0]), tuple(want[1])))
    assert len(tables) == 4
    again = _run(static, share, work, cost)  # the same bits on every run
    assert all(torch.equal(again[i], got[i]) for i in (0, 1, 3, 4, 5))  # (the lists: up to their counts, checked above)


def test_the_registered_operator_is_the_launcher():
    import vorta_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vorta_amd import ops
    tiers, work, cost = [2, 1, 0], [3.0, 1.0, 2.0], [0.5, 0.75, 1.0]
    sq_ref = torch.tensor(CRAFTED_REF, device=dev())
    sq_err = torch.tensor([CRAFTED[t] for t in tiers], device=dev())
    fids = {t: _fid(sq_ref, sq_err[i]) for i, t in enumerate(tiers)}
    want = ops.route_budget_tiers(fids, max_cost_share=0.5, work=work, tier_cost=dict(zip(tiers, cost)), cost_share=True)
    got = torch.ops.vorta.route_budget_tiers(sq_ref, sq_err, tiers, 0.5, work=work, tier_cost=cost)
    assert len(got) == 6
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.is_cuda
    assert all(torch.equal(got[i], want[i]) for i in (0, 1, 3, 4, 5))
    _check(_to_host(got), _host(tiers, sq_ref, list(sq_err), tuple(work), 0.5, dict(zip(tiers, cost))), "operator")
    _check(_to_host(torch.ops.vorta.route_budget_tiers(sq_ref, sq_err, tiers, 0.5)),
           _host(tiers, sq_ref, list(sq_err), (3.0, 2.0, 1.0), 0.5, None), "operator defaults")
    assert len(ops.route_budget_tiers(fids, max_cost_share=0.5)) == 5  # (without the share: the level is the fifth)
    with FakeTensorMode():
        fake = torch.ops.vorta.route_budget_tiers(torch.empty((8,), device="cuda"), torch.empty((3, 8, 3), device="cuda"),
                                                  tiers, 0.5, work=work, tier_cost=cost)
    assert [(tuple(f.shape), f.dtype) for f in fake] == [(tuple(t.shape), t.dtype) for t in want]
    with pytest.raises(ValueError, match="distinct"):
        torch.ops.vorta.route_budget_tiers(sq_ref, sq_err, [2, 2, 0], 0.5)
