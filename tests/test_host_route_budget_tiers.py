"""CPU: `vorta.patch.routes_within_cost_share`, the definition of the cost-budget rule over (precision tier, expert) pairs
(`ops.route_budget_tiers` / vorta_route_budget_tiers is held to it with `==` in tests/test_hip_route_budget_tiers.py).

Every rel below is k / 64 with sq_ref = 1 and sq_err = k^2 / 4096, so that the divide and the square root are exact in float32;
works and tier costs are small binary fractions, so that budgets can be met with equality on purpose.  The brute force
enumerates every assignment of finite-rel candidates of records drawn from the small value sets of
tests/test_hip_route_fidelity_tiers.py (NaN, inf and sq_ref == 0 among them) and holds the result to the two claims of the
rule: within the budget whenever anything is, and no assignment within the budget has a smaller largest rel than `level`.
Both claims rest on a cost that does not grow with r, which the rule's docstring ties to the tiers: a `native` tier, or full
attention in the last tier the dearest pair.  The draws take every tier order and cost table; a draw outside that condition
is held to what the rule promises there (a level whose state is within the budget, or the largest level)."""
import itertools
import math

import pytest
import torch

from test_hip_route_fidelity_tiers import COSTS, SQ_ERR, SQ_REF, TIER_ORDERS, WORKS, _fid, _fids

NAN, INF = float("nan"), float("inf")
HALF = {"i8pv": 0.5, "fp8pv": 0.75, "native": 1.0}


def k2(*ks):
    """sq_err entries whose rel against sq_ref = 1 is exactly k / 64 (None: NaN)"""
    return [NAN if k is None else k * k / 4096.0 for k in ks]


def _rule(fids, share, work=(3.0, 2.0, 1.0), cost=HALF):
    from vorta.patch import routes_within_cost_share
    return routes_within_cost_share(fids, share, dict(work=work), tier_cost=cost)


def _worked():
    i8 = _fid([1.0, 1.0], [k2(3, 7, 1), k2(5, 14, 1)])
    nat = _fid([1.0, 1.0], [k2(2, 6, None), k2(4, 12, None)])
    return {"i8pv": i8, "native": nat}


def test_worked_example_half_of_the_dense_cost():
    r = _rule(_worked(), 0.5)
    # state(0) costs 6, state(1/64) 3: the moves go head 0 (4.5), then head 1 (3.0, the budget met with equality)
    assert r.experts.tolist() == [0, 0] and r.tiers.tolist() == [2, 2]
    assert float(r.level) == 1 / 64 and float(r.cost_share) == 0.5
    assert r.experts.dtype == torch.int64 and r.level.dtype == torch.float32 and r.cost_share.dtype == torch.float32


def test_worked_example_four_tenths():
    r = _rule(_worked(), 0.4)
    # the costs at 2, 3, 4, 5 (/64) are 3, 2.5, 2.5, 2.0 against a budget of 2.4: r* = 5/64, r- = 4/64, only head 1 gets cheaper
    assert r.experts.tolist() == [1, 1] and r.tiers.tolist() == [2, 2]
    assert float(r.level) == 5 / 64 and float(r.cost_share) == float(torch.tensor(1 / 3, dtype=torch.float32))


def test_layers_are_routed_one_by_one():
    one = _worked()
    two = {t: _fid(torch.stack([f.sq_ref, f.sq_ref]), torch.stack([f.sq_err, f.sq_err.flip(0)])) for t, f in one.items()}
    r = _rule(two, 0.4)
    assert r.experts.shape == (2, 2) and r.level.shape == (2,) and r.cost_share.shape == (2,)
    assert r.experts[0].tolist() == [1, 1] and float(r.level[0]) == 5 / 64
    flipped = _rule({t: _fid(f.sq_ref, f.sq_err.flip(0)) for t, f in one.items()}, 0.4)
    assert r.experts[1].tolist() == flipped.experts.tolist() and float(r.level[1]) == float(flipped.level)


@pytest.mark.parametrize("share", [1.0, 1.5, INF])
def test_a_share_of_one_or_more_gives_state_zero(share):
    from vorta.patch import routes_from_fidelity_tiers, routes_within_cost_share
    g = torch.Generator().manual_seed(5)
    pick = lambda values, shape: torch.tensor(values)[torch.randint(0, len(values), shape, generator=g)]  # noqa: E731
    for tiers in [(0,), (2,), (2, 0), (1, 0), (2, 1, 0), (2, 1)]:
        for work in WORKS[:3]:
            fids = _fids(tiers, pick(SQ_REF, (7,)), [pick(SQ_ERR, (7, 3)) for _ in tiers])
            r = routes_within_cost_share(fids, share, dict(work=work))
            experts, tier_ids = routes_from_fidelity_tiers(fids, 0.0, dict(work=work))
            assert torch.equal(r.experts, experts) and torch.equal(r.tiers, tier_ids) and float(r.level) == 0.0
            assert float(r.cost_share) <= 1.0


def _rels(tiers, sq_ref, sq_errs):
    """[t][h][e] rel as Python floats, by the function under test's own float32 helper; the exact tier's full attention 0"""
    from vorta_amd.patch.fidelity import _rel_error_float32
    out = []
    for t, err in zip(tiers, sq_errs):
        cols = [_rel_error_float32(err[:, c], sq_ref) for c in range(3)]
        out.append([[0.0 if t == 0 else cols[2][h], cols[0][h], cols[1][h]] for h in range(sq_ref.numel())])
    return out


def _cost(pairs, c, T):
    total = 0.0
    for t in range(T):
        for e in range(3):
            n = sum(1 for p in pairs if p == (t, e))
            if n:
                total = total + n * c[t][e]
    return total


@pytest.mark.parametrize("n_tiers", [1, 2])
@pytest.mark.parametrize("H", [1, 2, 3, 4])
def test_brute_force_over_every_assignment(H, n_tiers):
    from vorta_amd import ops
    from vorta.patch import routes_within_cost_share
    g = torch.Generator().manual_seed(1000 * H + n_tiers)
    pick = lambda values, shape: torch.tensor(values)[torch.randint(0, len(values), shape, generator=g)]  # noqa: E731
    choose = lambda values: values[int(torch.randint(0, len(values), (1,), generator=g))]  # noqa: E731
    moved = over = claims = 0
    for _ in range(40 if H < 4 else 16):
        tiers, work, cost = choose(TIER_ORDERS[n_tiers]), choose(WORKS), choose(COSTS)
        sq_ref, sq_errs = pick(SQ_REF, (H,)), [pick(SQ_ERR, (H, 3)) for _ in range(n_tiers)]
        share = choose([0.1, 0.25, 1 / 3, 0.5, 0.59, 0.75, 0.9])
        r = routes_within_cost_share(_fids(tiers, sq_ref, sq_errs), share, dict(work=work), tier_cost=cost)
        T = n_tiers
        tc = [(ops.DEFAULT_TIER_COST[ops.TIER_NAMES[t]] if cost is None else cost[t]) for t in tiers]
        c = [[work[e] * tc[t] for e in range(3)] for t in range(T)]
        budget = share * (H * c[T - 1][0])
        rel = _rels(tiers, sq_ref, sq_errs)
        # per head its finite-rel candidates; a head without one is on (T-1, 0) in every assignment, its error not counted
        options = []
        for h in range(H):
            cands = [((t, e), rel[t][h][e]) for t in range(T) for e in range(3) if math.isfinite(rel[t][h][e])]
            options.append(cands or [((T - 1, 0), 0.0)])
        got = [(list(tiers).index(int(t)), int(e)) for e, t in zip(r.experts.tolist(), r.tiers.tolist())]
        got_cost, level = _cost(got, c, T), float(r.level)
        case = f"tiers={tiers} work={work} cost={cost} share={share} ref={sq_ref.tolist()} errs={[e.tolist() for e in sq_errs]}"
        assert float(r.cost_share) == float(torch.tensor(got_cost / (H * c[T - 1][0]), dtype=torch.float64).float()), case
        for h, pair in enumerate(got):  # every head is on a candidate within the level ...
            # (... or, without a `native` tier, on the fallback (T-1, 0), which is not covered, as in the bound rule)
            assert dict(options[h]).get(pair, INF) <= level or (0 not in tiers and pair == (T - 1, 0)), case
        # the two claims hold where the cost of a state does not grow with r: with a `native` tier, or with full attention
        # in the last tier the dearest pair (the docstring of the rule); every draw is held to the rest
        monotone = 0 in tiers or all(c[t][e] <= c[T - 1][0] for t in range(T) for e in range(3))
        any_within = False
        for choice in itertools.product(*options):
            if not _cost([p for p, _ in choice], c, T) > budget:
                any_within = True
                if monotone:
                    assert not max(x for _, x in choice) < level, f"{case}: {choice} is within the budget under level {level}"
        if any_within and monotone:
            assert not got_cost > budget, f"{case}: {got} costs {got_cost} > {budget} although an assignment is within"
        if not any_within and monotone:
            over += 1
            assert float(r.cost_share) > share, case
        if not monotone:  # another order: still a level whose state is within the budget, or the largest level
            top = max([0.0] + [x for cands in options for _, x in cands])
            assert not got_cost > budget or level == top, case
        moved += level > 0
        claims += monotone
    assert moved >= 5 and claims >= 8, "the draws do exercise the rule"


def test_a_growing_share_never_raises_the_level():
    from vorta.patch import routes_within_cost_share
    g = torch.Generator().manual_seed(11)
    pick = lambda values, shape: torch.tensor(values)[torch.randint(0, len(values), shape, generator=g)]  # noqa: E731
    distinct = set()
    for tiers in [(2, 0), (2, 1, 0), (1,), (0,)]:
        for work in WORKS[:4]:
            fids = _fids(tiers, pick(SQ_REF, (9,)), [pick(SQ_ERR, (9, 3)) for _ in tiers])
            levels = [float(routes_within_cost_share(fids, s, dict(work=work)).level) for s in (0.05, 0.2, 0.35, 0.5, 0.65, 0.8, 1.0)]
            assert all(a >= b for a, b in zip(levels, levels[1:])), (tiers, work, levels)
            distinct.update(levels)
    assert len(distinct) >= 3


def test_a_level_is_the_rel_of_a_head_that_was_moved_to_it():
    """on records whose rel are NOT representable fractions: the level and the rel it came from are one number (both from the
    correctly rounded float32 divide and square root), so the head that sits at the level qualifies at it -- with a square root
    that is an ulp off on either side the state at a level would miss its own head and the level would read one step high"""
    from vorta.patch import routes_within_cost_share
    from vorta_amd.patch.fidelity import _rel_error_float32
    g = torch.Generator().manual_seed(3)
    hits = 0
    for _ in range(40):
        sq_ref = torch.rand(6, generator=g) + 0.5
        errs = [torch.rand((6, 3), generator=g) * 0.3 for _ in range(2)]
        r = routes_within_cost_share(_fids((2, 0), sq_ref, errs), 0.45, dict(work=(3.0, 1.0, 1.5)))
        level = float(r.level)
        if level == 0 or float(r.cost_share) > 0.45:
            continue
        rels = []
        for h, (e, t) in enumerate(zip(r.experts.tolist(), r.tiers.tolist())):
            err = errs[(2, 0).index(t)]
            rels.append(0.0 if (e, t) == (0, 0) else _rel_error_float32(err[:, 2 if e == 0 else e - 1], sq_ref)[h])
        assert max(rels) == level, (rels, level)
        hits += 1
    assert hits >= 20


def test_ties_at_one_rel_move_the_lowest_heads_first_and_equality_is_within():
    # four heads, all with the coreset at 4/64 and the sliding tile far off; work (4, 2, 1): dense 16, a move saves 2
    fid = {"native": _fid([1.0] * 4, [k2(4, 63, None)] * 4)}
    r = _rule(fid, 0.75, work=(4.0, 2.0, 1.0))  # budget 12: two moves, 16 -> 14 -> 12, met with equality
    assert r.experts.tolist() == [1, 1, 0, 0] and float(r.level) == 4 / 64 and float(r.cost_share) == 0.75
    r = _rule(fid, 0.75 - 2.0 ** -20, work=(4.0, 2.0, 1.0))  # a hair under: a third move
    assert r.experts.tolist() == [1, 1, 1, 0] and float(r.level) == 4 / 64
    r = _rule(fid, 0.875, work=(4.0, 2.0, 1.0))  # budget 14: one move
    assert r.experts.tolist() == [1, 0, 0, 0] and float(r.cost_share) == 0.875


def test_an_equal_cost_candidate_moves_no_head():
    from vorta.patch import routes_from_fidelity_tiers
    # work (4, 2, 2): head 0's sliding tile (3/64) costs what its coreset (1/64) does; head 1's sliding tile (3/64) is its step
    fid = {"native": _fid([1.0, 1.0], [k2(1, 3, None), k2(5, 3, None)])}
    r = _rule(fid, 0.5, work=(4.0, 2.0, 2.0))  # budget 4: state(1/64) costs 6, state(3/64) 4
    assert float(r.level) == 3 / 64 and float(r.cost_share) == 0.5
    assert r.experts.tolist() == [1, 2], "head 0 stays on its coreset: the sliding tile is no cheaper"
    assert routes_from_fidelity_tiers(fid, 3 / 64, dict(work=(4.0, 2.0, 2.0)))[0].tolist() == [2, 2]  # (state(r*) itself moves it)


def test_without_an_exact_tier_and_where_the_candidates_run_out():
    # i8pv alone: head 1 has no candidate at all and stays on the fallback, full attention in the last (only) tier
    fid = {"i8pv": _fid([1.0, 1.0], [k2(2, 3, 1), [NAN, INF, NAN]])}
    r = _rule(fid, 0.5)  # dense 3, budget 1.5; the states cost 3, 3, 2.5, 2.0: no level is within
    assert r.experts.tolist() == [2, 0] and r.tiers.tolist() == [2, 2]
    assert float(r.level) == 3 / 64, "the largest level"
    assert float(r.cost_share) == float(torch.tensor(2 / 3, dtype=torch.float32)) and float(r.cost_share) > 0.5
    r = _rule(fid, 0.75)  # budget 2.25: r* = 3/64, head 0 steps from the coreset to the sliding tile
    assert r.experts.tolist() == [2, 0] and float(r.level) == 3 / 64
    r = _rule(fid, 0.875)  # budget 2.625: the coreset is enough
    assert r.experts.tolist() == [1, 0] and float(r.level) == 2 / 64
    r = _rule(fid, 1.0)  # state(0): nothing is exact, both heads on the fallback
    assert r.experts.tolist() == [0, 0] and float(r.level) == 0.0 and float(r.cost_share) == 1.0


def test_one_tier_is_not_the_flop_budget_rule():
    """`routes_from_fidelity(max_flops_share=...)` gives a head one candidate (its smaller-rel sparse expert); this rule lets a
    head step down twice"""
    from vorta.patch import routes_from_fidelity
    f = _fid([1.0], [k2(1, 2, None)])
    old = routes_from_fidelity(f, geometry=dict(work=(3.0, 2.0, 1.0)), max_flops_share=0.4)
    new = _rule({"native": f}, 0.4)
    assert old.tolist() == [1] and new.experts.tolist() == [2] and float(new.level) == 2 / 64


def test_refusals():
    from vorta.patch import routes_within_cost_share
    f = _fid([1.0], [k2(1, 2, 3)])
    for share in (0.0, -0.5, NAN, None):
        with pytest.raises(ValueError, match="max_cost_share"):
            routes_within_cost_share({"i8pv": f}, share)
    with pytest.raises(ValueError, match="tier"):
        routes_within_cost_share({3: f}, 0.5)
    with pytest.raises(ValueError, match="tier"):
        routes_within_cost_share({"int4": f}, 0.5)
    with pytest.raises(ValueError, match="distinct"):
        routes_within_cost_share({"i8pv": f, 2: f}, 0.5)
    with pytest.raises(ValueError, match="mapping"):
        routes_within_cost_share([f], 0.5)
    for bad in (0.0, -1.0, INF, NAN):
        with pytest.raises(ValueError, match="tier_cost"):
            routes_within_cost_share({"i8pv": f}, 0.5, tier_cost={"i8pv": bad})
