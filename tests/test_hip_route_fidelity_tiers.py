"""GPU: `ops.route_fidelity_tiers` (vorta_route_fidelity_tiers) against the host rule, `vorta.patch.routes_from_fidelity_tiers`,
which is the definition.  The host rule is evaluated on CPU copies of the records; the expert table, the tier table, the
counts, every list up to its count and the cost share must be EQUAL -- no tolerance: rel is two correctly rounded float32
operations, a cost one double product.

Crafted records (ties across and within tiers, NaN, inf, sq_ref == 0, bound 0, no exact tier); random records with errors
from a small set, so that ties are common, at H in {1, 5, 24, 40, 1024} x 1..3 tiers in every order (so the exact tier sits at
every index, and nowhere); the sentinel past a count; one tier against `ops.route_fidelity`; the error codes; the operator."""
import ctypes as C
import itertools

import pytest
import torch

from _util import dev

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
SQ_REF = [0.0, 1.0, 4.0, 16.0, 16.0, 16.0]
SQ_ERR = [0.0, 0.25, 1.0, 1.0, 4.0, 9.0, 9.0, 16.0, 3.0, 1e-30, NAN, INF]
WORKS = [(3.0, 2.0, 1.0), (3.0, 1.0, 2.0), (3.0, 2.0, 2.0), (5.0, 5.0, 1.5), (4.0, 6.0, 1.0), (2.0, 3.0, 2.0),
         (1.2176e15, 3.1e14, 2.9e14), (0.7, 0.1, 0.3)]
BOUNDS = [0.0, 0.25, 0.5, 0.75, 1.0, 0.4330127, 3.0, INF]
# costs that tie across tiers with the works above (2 * 0.5 == 1 * 1.0, 3 * 0.5 == 1.5 * 1.0), the default, and odd ones
COSTS = [None, {0: 1.0, 1: 1.0, 2: 1.0}, {0: 1.0, 1: 0.5, 2: 0.5}, {0: 1.0, 1: 0.75, 2: 0.5}, {0: 0.3, 1: 0.7, 2: 1.9},
         {0: 1.0, 1: 0.8, 2: 1.0 / 3.0}]
TIER_ORDERS = {n: list(itertools.permutations((0, 1, 2), n)) for n in (1, 2, 3)}


def _fid(sq_ref, sq_err, device=None):
    from vorta_amd.ops import ExpertFidelity
    sq_ref, sq_err = (torch.as_tensor(x, dtype=torch.float32) for x in (sq_ref, sq_err))
    if device is not None:
        sq_ref, sq_err = sq_ref.to(device), sq_err.to(device)
    return ExpertFidelity(sq_ref, sq_ref.sqrt(), sq_err, sq_err.sqrt(), None, 128)


def _record(H, n_tiers, seed):
    """(tier ids, sq_ref, per-tier sq_err, work, bound, tier_cost): every column drawn, column 2 included"""
    g = torch.Generator().manual_seed(100000 * n_tiers + 1000 * H + seed)
    pick = lambda values, shape: torch.tensor(values)[torch.randint(0, len(values), shape, generator=g)]  # noqa: E731
    choose = lambda values: values[int(torch.randint(0, len(values), (1,), generator=g))]  # noqa: E731
    return (choose(TIER_ORDERS[n_tiers]), pick(SQ_REF, (H,)), [pick(SQ_ERR, (H, 3)) for _ in range(n_tiers)], choose(WORKS),
            choose(BOUNDS), choose(COSTS))


def _fids(tiers, sq_ref, sq_errs, device=None):
    return {t: _fid(sq_ref, e, device) for t, e in zip(tiers, sq_errs)}


def _host(tiers, sq_ref, sq_errs, work, bound, cost):
    from vorta_amd.patch import routes_from_fidelity_tiers
    experts, tier_ids = routes_from_fidelity_tiers(_fids(tiers, sq_ref.cpu(), [e.cpu() for e in sq_errs]), bound, dict(work=work),
                                                   tier_cost=cost)
    return experts.tolist(), [list(tiers).index(t) for t in tier_ids.tolist()]  # the device speaks the caller's tier INDEX


def _check(got, want, tiers, work, cost, case):
    """one call's device outputs (already on the host) against the host tables"""
    from vorta_amd import ops
    expert, tier, lists, counts, share = got
    want_expert, want_tier = want
    H, T = len(want_expert), len(tiers)
    assert expert == want_expert, f"{case}: expert table {expert} != host {want_expert}"
    assert tier == want_tier, f"{case}: tier table {tier} != host {want_tier}"
    costs = [(ops.DEFAULT_TIER_COST[ops.TIER_NAMES[t]] if cost is None else cost[t]) for t in tiers]
    total = 0.0
    for t in range(T):
        for e in range(3):
            heads = [h for h in range(H) if want_tier[h] == t and want_expert[h] == e]
            assert counts[t][e] == len(heads), f"{case}: count of tier index {t} expert {e}: {counts}"
            assert lists[t][e][:len(heads)] == heads, f"{case}: list of tier index {t} expert {e}"
            total = total + len(heads) * (work[e] * costs[t])
    formula = total / (H * (work[0] * costs[-1]))
    assert share == float(torch.tensor(formula, dtype=torch.float64).float()), f"{case}: share {share} != {formula}"


def _run(fids, bound, work, cost):
    from vorta_amd import ops
    return ops.route_fidelity_tiers(fids, max_rel_error=bound, work=work, tier_cost=cost, cost_share=True)


def _to_host(got):
    return [t.cpu().tolist() for t in got[:4]] + [float(got[4])]


CRAFTED_REF = [16.0, 1.0, 1.0, 0.0, 0.0, 16.0, 16.0, 16.0]
CRAFTED_I8 = [[9.0, 100.0, 100.0],   # coreset exactly AT the bound 0.75
              [NAN, NAN, NAN],        # NaN meets no bound: the exact tier's full attention, or the fallback
              [INF, INF, INF],
              [0.0, 0.0, 0.0],        # sq_ref == 0 and sq_err == 0: rel 0, everything qualifies
              [1.0, 2.0, 1.0],        # sq_ref == 0 and sq_err > 0: inf
              [1.0, 4.0, 1.0],        # 0.25, 0.5, 0.25
              [16.0, 25.0, 9.0],      # sparse over the bound, full attention in this tier AT it
              [100.0, 100.0, 100.0]]
CRAFTED_F8 = [[100.0, 100.0, 1.0], [NAN, 0.25, NAN], [INF, INF, 0.0], [1.0, 0.0, 1.0], [0.0, 0.0, 0.0], [100.0, 1.0, 100.0],
              [16.0, 25.0, 100.0], [100.0, 100.0, 9.0]]
CRAFTED_NAT = [[100.0, 1.0, NAN], [NAN, NAN, NAN], [INF, INF, 5.0], [1.0, 1.0, 0.0], [1.0, 1.0, 1.0], [100.0, 100.0, 100.0],
               [9.0, 25.0, NAN], [100.0, 100.0, INF]]
CRAFTED = {2: CRAFTED_I8, 1: CRAFTED_F8, 0: CRAFTED_NAT}


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("work", WORKS[:4])
def test_crafted_records(work, cost):
    for n in (1, 2, 3):
        for tiers in TIER_ORDERS[n]:
            errs = [torch.tensor(CRAFTED[t]) for t in tiers]
            ref = torch.tensor(CRAFTED_REF)
            for bound in (0.0, 0.75, 0.7499999, INF):
                got = _run(_fids(tiers, ref, errs, dev()), bound, work, cost)
                assert all(t.is_cuda for t in got) and [t.dtype for t in got] == [torch.int32] * 4 + [torch.float32]
                _check(_to_host(got), _host(tiers, ref, errs, work, bound, cost), tiers, work, cost,
                       f"crafted tiers={tiers} bound={bound} work={work} cost={cost}")


def test_crafted_ties_and_the_fallback_by_hand():
    ref, i8, f8, nat = (torch.tensor(x) for x in (CRAFTED_REF, CRAFTED_I8, CRAFTED_F8, CRAFTED_NAT))
    same = {0: 1.0, 1: 1.0, 2: 1.0}
    # equal costs across tiers: head 3 (its sliding tile at rel 0 in both 8-bit tiers) takes it in tier index 0, whichever of
    # the two that is
    for tiers in [t for t in TIER_ORDERS[3] if t[0] != 0]:
        got = _to_host(_run(_fids(tiers, ref, [torch.tensor(CRAFTED[t]) for t in tiers], dev()), 0.75, (3.0, 2.0, 1.0), same))
        assert (got[0][3], got[1][3]) == (2, 0), (tiers, got)
    # equal costs within a tier: head 5 in i8pv alone, coreset (0.25) and sliding tile (0.5) at equal work: expert 2
    got = _to_host(_run(_fids((2,), ref, [i8], dev()), 0.75, (3.0, 2.0, 2.0), None))
    assert got[0][5] == 2
    # no exact tier: heads 1, 2, 4, 7 have no candidate under 0.75 in i8pv alone -> full attention in the last (only) tier
    assert [got[0][h] for h in (1, 2, 4, 7)] == [0] * 4 and got[1] == [0] * 8
    # ... and with (i8pv, fp8pv) head 7 (fp8pv full attention at 0.75) and head 1 (fp8pv sliding tile) are found there
    got = _to_host(_run(_fids((2, 1), ref, [i8, f8], dev()), 0.75, (3.0, 2.0, 1.0), None))
    assert (got[0][7], got[1][7]) == (0, 1) and (got[0][1], got[1][1]) == (2, 1)
    # the exact tier: head 1 under (i8pv, native) goes to native's full attention although its column 2 is NaN
    got = _to_host(_run(_fids((2, 0), ref, [i8, nat], dev()), 0.75, (3.0, 2.0, 1.0), None))
    assert (got[0][1], got[1][1]) == (0, 1)
    # bound 0: exact candidates alone
    got = _to_host(_run(_fids((2, 0), ref, [i8, nat], dev()), 0.0, (3.0, 2.0, 1.0), None))
    assert got[0] == [0, 0, 0, 2, 0, 0, 0, 0] and got[1] == [1, 1, 1, 0, 1, 1, 1, 1]


@pytest.mark.parametrize("n_tiers", [1, 2, 3])
@pytest.mark.parametrize("H", [1, 5, 24, 40, 1024])
def test_random_records_equal_the_host_rule(H, n_tiers):
    seeds = 12 if H == 1024 else 120
    cases, outs = [], []
    for seed in range(seeds):
        tiers, sq_ref, sq_errs, work, bound, cost = _record(H, n_tiers, seed)
        cases.append((tiers, sq_ref, sq_errs, work, bound, cost))
        outs.append(_run(_fids(tiers, sq_ref, sq_errs, dev()), bound, work, cost))
    torch.cuda.synchronize()
    tables = set()
    for seed, (case, got) in enumerate(zip(cases, outs)):
        tiers, sq_ref, sq_errs, work, bound, cost = case
        want = _host(*case)
        _check(_to_host(got), want, tiers, work, cost, f"H={H} seed={seed} tiers={tiers} bound={bound} work={work} cost={cost}")
        tables.add((tuple(want[0]), tuple(want[1])))
    assert len(tables) >= (2 if H == 1 else 10)  # the draws do exercise the rule


@pytest.mark.parametrize("H", [1, 5, 24, 40, 1024])
def test_one_tier_equals_route_fidelity(H):
    """one exact tier: the expert table, the lists up to their counts and the counts of `ops.route_fidelity` on the record,
    wherever both sparse experts are cheaper than full attention (route_fidelity never weighs full attention's cost)"""
    from vorta_amd import ops
    for seed in range(24):
        _, sq_ref, sq_errs, work, bound, _ = _record(H, 1, seed)
        if not (work[1] < work[0] and work[2] < work[0]):
            continue
        fid = _fid(sq_ref, sq_errs[0], dev())
        expert, tier, lists, counts = ops.route_fidelity_tiers({"native": fid}, max_rel_error=bound, work=work)
        old_expert, old_lists, old_counts = ops.route_fidelity(fid, max_rel_error=bound, work=work)
        assert torch.equal(expert, old_expert) and torch.equal(counts[0], old_counts) and not bool(tier.any()), (H, seed)
        for e, n in enumerate(old_counts.tolist()):
            assert torch.equal(lists[0, e, :n], old_lists[e, :n]), (H, seed, e)


def _raw_args(ref_t, err_t, expert, tier, lists, counts, **kw):
    from vorta_amd import _C
    a = _C.RouteFidelityTiersArgs()
    a.struct_size, a.heads, a.n_tiers, a.exact_tier, a.mode, a.max_rel_error = C.sizeof(a), ref_t.numel(), 2, 1, 0, 0.75
    a.sq_ref, a.sq_err = ref_t.data_ptr(), err_t.data_ptr()
    a.expert_of_head, a.tier_of_head = expert.data_ptr(), tier.data_ptr()
    a.head_lists, a.head_counts = lists.data_ptr(), counts.data_ptr()
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
    lib, stream = _C.lib(), torch.cuda.current_stream().cuda_stream
    bad = [dict(heads=1025), dict(heads=0), dict(n_tiers=0), dict(n_tiers=4), dict(exact_tier=-2), dict(exact_tier=2),
           dict(sq_ref=None), dict(sq_err=None), dict(expert_of_head=None), dict(tier_of_head=None), dict(head_lists=None),
           dict(head_counts=None), dict(max_rel_error=-0.5), dict(max_rel_error=NAN), dict(mode=1), dict(mode=2),
           dict(work=(1, 0.0)), dict(work=(0, INF)), dict(work=(2, NAN)), dict(tier_cost=(0, 0.0)), dict(tier_cost=(1, -1.0)),
           dict(tier_cost=(1, INF)), dict(tier_cost=(0, NAN)), dict(n_tiers=3, exact_tier=1),  # (the third cost is NaN)
           dict(struct_size=C.sizeof(_C.RouteFidelityTiersArgs) - 8)]
    for kw in bad:
        assert lib.vorta_route_fidelity_tiers(C.byref(_raw_args(sq_ref, sq_err, *outs, **kw)), stream) == _C.VORTA_EINVAL, kw
    assert lib.vorta_route_fidelity_tiers(None, stream) == _C.VORTA_EINVAL
    torch.cuda.synchronize()
    assert all(bool((t == -7).all()) for t in outs), "a refused call wrote its outputs"
    assert lib.vorta_route_fidelity_tiers(C.byref(_raw_args(sq_ref, sq_err, *outs)), stream) == _C.VORTA_OK  # the same block
    torch.cuda.synchronize()
    want = _host((2, 0), sq_ref, list(sq_err), (3.0, 2.0, 1.0), 0.75, {2: 0.59, 0: 1.0})
    expert, tier, lists, counts = (t.cpu().tolist() for t in outs)
    assert (expert, tier) == want
    for t in range(2):
        for e in range(3):
            heads = [h for h in range(H) if want[1][h] == t and want[0][h] == e]
            assert counts[t][e] == len(heads) and lists[t][e] == heads + [-7] * (H - len(heads)), (t, e)  # past the count: not written
    assert sum(sum(c) for c in counts) == H and max(max(c) for c in counts) < H  # (some sentinel does survive)
    fid = _fid(CRAFTED_REF, CRAFTED_I8, dev())
    big = _fid([1.0] * 1025, [[0.0, 0.0, NAN]] * 1025, dev())
    with pytest.raises(ValueError, match="vorta_route_fidelity_tiers"):
        ops.route_fidelity_tiers({"i8pv": big}, max_rel_error=0.5)
    with pytest.raises(ValueError, match="vorta_route_fidelity_tiers"):
        ops.route_fidelity_tiers({"i8pv": fid}, max_rel_error=-1.0)
    with pytest.raises(ValueError, match="vorta_route_fidelity_tiers"):
        ops.route_fidelity_tiers({"i8pv": fid}, max_rel_error=0.5, work=(3.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="max_flops_share"):
        ops.route_fidelity_tiers({"i8pv": fid}, max_flops_share=0.5)
    with pytest.raises(ValueError, match="tier_cost"):
        ops.route_fidelity_tiers({"i8pv": fid}, max_rel_error=0.5, tier_cost={"i8pv": 0.0})
    with pytest.raises(ValueError, match="tier"):
        ops.route_fidelity_tiers({3: fid}, max_rel_error=0.5)
    with pytest.raises(ValueError, match="ONE layer"):
        ops.route_fidelity_tiers({"i8pv": _fid([CRAFTED_REF], [CRAFTED_I8], dev())}, max_rel_error=0.5)


def test_graph_replay_follows_the_statistics_in_the_buffers():
    H, tiers = 40, (2, 1, 0)
    _, sq_ref, sq_errs, work, _, cost = _record(H, 3, 0)
    static = _fids(tiers, sq_ref.to(dev()), [e.to(dev()) for e in sq_errs])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        _run(static, 0.5, work, cost)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = _run(static, 0.5, work, cost)
    tables = set()
    for seed in (0, 1, 2, 3):
        _, new_ref, new_errs, _, _, _ = _record(H, 3, seed)
        static[tiers[0]].sq_ref.copy_(new_ref)
        for t, e in zip(tiers, new_errs):
            static[t].sq_err.copy_(e)
        graph.replay()
        torch.cuda.synchronize()
        want = _host(tiers, new_ref, new_errs, work, 0.5, cost)
        _check(_to_host(got), want, tiers, work, cost, f"replay seed {seed}")
        tables.add((tuple(want[0]), tuple(want[1])))
    assert len(tables) == 4
    again = _run(static, 0.5, work, cost)  # the same bits on every run
    assert all(torch.equal(again[i], got[i]) for i in (0, 1, 3, 4))  # (the lists: up to their counts, checked above)


def test_the_registered_operator_is_the_launcher():
    import vorta_amd.torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    from vorta_amd import ops
    tiers, work, cost = [2, 1, 0], [3.0, 1.0, 2.0], [0.5, 0.75, 1.0]
    sq_ref = torch.tensor(CRAFTED_REF, device=dev())
    sq_err = torch.tensor([CRAFTED[t] for t in tiers], device=dev())
    fids = {t: _fid(sq_ref, sq_err[i]) for i, t in enumerate(tiers)}
    want = ops.route_fidelity_tiers(fids, max_rel_error=0.75, work=work, tier_cost=dict(zip(tiers, cost)), cost_share=True)
    got = torch.ops.vorta.route_fidelity_tiers(sq_ref, sq_err, tiers, 0.75, work=work, tier_cost=cost)
    assert len(got) == 5
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.is_cuda
    _check(_to_host(got), _host(tiers, sq_ref, list(sq_err), tuple(work), 0.75, dict(zip(tiers, cost))), tiers, work,
           dict(zip(tiers, cost)), "operator")
    _check(_to_host(torch.ops.vorta.route_fidelity_tiers(sq_ref, sq_err, tiers, 0.75)),
           _host(tiers, sq_ref, list(sq_err), (3.0, 2.0, 1.0), 0.75, None), tiers, (3.0, 2.0, 1.0), None, "operator defaults")
    with FakeTensorMode():
        fake = torch.ops.vorta.route_fidelity_tiers(torch.empty((8,), device="cuda"), torch.empty((3, 8, 3), device="cuda"),
                                                    tiers, 0.75, work=work, tier_cost=cost)
    assert [(tuple(f.shape), f.dtype) for f in fake] == [(tuple(t.shape), t.dtype) for t in want]
    with pytest.raises(ValueError, match="distinct"):
        torch.ops.vorta.route_fidelity_tiers(sq_ref, sq_err, [2, 2, 0], 0.75)
