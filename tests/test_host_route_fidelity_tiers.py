"""No GPU: `vorta.patch.routes_from_fidelity_tiers`, the definition of the rule over (precision tier, expert) pairs that
vorta_route_fidelity_tiers applies on the device, on hand-made records.

A record per tier: column 0 coreset, column 1 sliding tile, column 2 full attention, all in that tier's precision against the
one dense reference.  Sums of squares whose ratios are squares of short binary fractions, so rel is exact."""
import pytest
import torch

NAN, INF = float("nan"), float("inf")


def _fid(sq_ref, sq_err):
    from vorta_amd.ops import ExpertFidelity
    sq_ref, sq_err = (torch.as_tensor(x, dtype=torch.float32) for x in (sq_ref, sq_err))
    return ExpertFidelity(sq_ref, sq_ref.sqrt(), sq_err, sq_err.sqrt(), None, 128)


def _route(fids, bound, work=(3.0, 2.0, 1.0), **kw):
    from vorta_amd.patch import routes_from_fidelity_tiers
    experts, tiers = routes_from_fidelity_tiers(fids, bound, dict(work=work), **kw)
    assert experts.dtype == tiers.dtype == torch.int64
    return experts.tolist(), tiers.tolist()


REF = [16.0, 1.0, 1.0, 0.0, 0.0, 16.0, 16.0]
ERR = [[9.0, 100.0, NAN],    # coreset exactly AT the bound 0.75
       [NAN, NAN, NAN],
       [INF, INF, NAN],
       [0.0, 0.0, NAN],      # sq_ref == 0 and sq_err == 0: rel 0
       [1.0, 2.0, NAN],      # sq_ref == 0 and sq_err > 0: inf
       [1.0, 4.0, NAN],      # 0.25 and 0.5
       [16.0, 25.0, NAN]]    # 1 and 1.25


@pytest.mark.parametrize("work", [(3.0, 2.0, 1.0), (3.0, 1.0, 2.0), (3.0, 2.0, 2.0), (1.2176e15, 3.1e14, 2.9e14)])
@pytest.mark.parametrize("bound", [0.0, 0.25, 0.5, 0.75, 0.7499999, 1.0, 3.0, INF])
@pytest.mark.parametrize("tier", ["native", 0])
def test_one_exact_tier_is_routes_from_fidelity(work, bound, tier):
    """one tier whose full attention is the reference, both sparse experts cheaper than it: the rule of today, and the layer
    axis carried"""
    from vorta_amd.patch import routes_from_fidelity
    fid = _fid([REF, REF[::-1]], [ERR, ERR[::-1]])
    experts, tiers = _route({tier: fid}, bound, work)
    assert experts == routes_from_fidelity(fid, bound, dict(work=work)).tolist()
    assert tiers == [[0] * 7] * 2
    if work == (3.0, 2.0, 1.0) and bound == 0.75:
        assert experts[0] == [1, 0, 0, 2, 0, 2, 0]
        from vorta_amd.patch import routes_from_fidelity_tiers
        assert routes_from_fidelity_tiers({tier: fid}, bound)[0].tolist() == experts  # no geometry: work (3, 2, 1)


def test_equal_costs_across_tiers_take_the_lower_tier_index():
    fid = _fid([16.0], [[1.0, 1.0, 1.0]])  # every candidate at 0.25
    same = {"i8pv": 1.0, "fp8pv": 1.0, "native": 1.0}
    assert _route({"i8pv": fid, "fp8pv": fid, "native": fid}, 0.5, tier_cost=same) == ([2], [2])   # index 0 is i8pv
    assert _route({"fp8pv": fid, "i8pv": fid, "native": fid}, 0.5, tier_cost=same) == ([2], [1])   # index 0 is fp8pv
    assert _route({2: fid, 1: fid}, 0.5, tier_cost={2: 0.5, 1: 0.5}) == ([2], [2])
    # a cost tie between DIFFERENT experts of different tiers: (tier 0, coreset) 2 * 0.5 == (tier 1, sliding) 1 * 1.0
    only_coreset = _fid([16.0], [[1.0, 100.0, 100.0]])
    assert _route({"i8pv": only_coreset, "native": fid}, 0.5, tier_cost={"i8pv": 0.5, "native": 1.0}) == ([1], [2])
    # and a strictly cheaper candidate in a later tier wins
    assert _route({"i8pv": only_coreset, "native": fid}, 0.5, tier_cost={"i8pv": 0.75, "native": 1.0}) == ([2], [0])


def test_equal_costs_within_a_tier_take_the_larger_expert():
    fid = _fid([16.0, 16.0], [[1.0, 1.0, 1.0], [1.0, 100.0, 1.0]])
    assert _route({"i8pv": fid}, 0.5, (3.0, 2.0, 2.0)) == ([2, 1], [2, 2])
    assert _route({"i8pv": fid}, 0.5, (2.0, 2.0, 2.0)) == ([2, 1], [2, 2])   # coreset ties with full attention: the larger id
    assert _route({"i8pv": fid}, 0.5, (1.0, 2.0, 2.0)) == ([0, 0], [2, 2])   # full attention is the cheapest


def test_nan_columns_and_a_zero_reference():
    i8 = _fid([16.0, 16.0, 0.0, 0.0, 16.0],
              [[NAN, NAN, NAN],      # nothing qualifies in i8pv: native's full attention (rel 0) does
               [NAN, 1.0, NAN],      # the sliding tile does
               [0.0, 5.0, 0.0],      # sq_ref == 0: coreset and full at rel 0, the sliding tile at inf
               [1.0, 1.0, 1.0],      # sq_ref == 0, every error positive: inf everywhere
               [NAN, NAN, 1.0]])     # full attention in i8pv
    nat = _fid([16.0] * 5, [[NAN, NAN, NAN]] * 5)  # (its sq_ref is not the one that counts: the first record's is)
    assert _route({"i8pv": i8, "native": nat}, 0.5) == ([0, 2, 1, 0, 0], [0, 2, 2, 0, 2])
    # inf <= inf: heads 2 and 3 take the sliding tile, the cheapest; NaN still meets nothing
    assert _route({"i8pv": i8, "native": nat}, INF) == ([0, 2, 2, 2, 0], [0, 2, 2, 2, 2])


def test_bound_zero():
    i8 = _fid([16.0, 16.0, 16.0], [[0.0, 1.0, 1.0], [1.0, 1.0, 0.0], [1.0, 1.0, 1e-30]])
    nat = _fid([16.0] * 3, [[1.0, 1.0, NAN]] * 3)
    # exact candidates alone: i8pv's coreset; i8pv's full attention (0.59 * 3 = 1.77 against native's 3); native's, the reference
    assert _route({"i8pv": i8, "native": nat}, 0.0) == ([1, 0, 0], [2, 2, 0])
    # ... and an exact sparse expert in the input dtype is cheaper than any of them: 1.0 against 2 * 0.59 and 1.77
    exact = _fid([16.0] * 3, [[1.0, 0.0, NAN]] * 3)
    assert _route({"i8pv": i8, "native": exact}, 0.0) == ([2, 2, 2], [0, 0, 0])
    assert _route({"i8pv": i8}, 0.0) == ([1, 0, 0], [2, 2, 2])  # head 2: nothing exact, the fallback


def test_no_exact_tier_and_every_candidate_over_the_bound_is_full_attention_in_the_last_tier():
    over = _fid([16.0, 16.0], [[16.0, 16.0, 16.0], [NAN, INF, 4.0]])
    assert _route({"i8pv": over, "fp8pv": over}, 0.25) == ([0, 0], [1, 1])
    assert _route({"fp8pv": over, "i8pv": over}, 0.25) == ([0, 0], [2, 2])
    assert _route({"i8pv": over}, 0.25) == ([0, 0], [2, 2])
    # head 1: full attention is AT the bound in both tiers: the cheaper tier, 3 * 0.59 against 3 * 0.80, although it is listed second
    assert _route({"fp8pv": over, "i8pv": over}, 0.5) == ([0, 0], [2, 2])


def test_the_default_costs_are_the_published_ratios():
    from vorta_amd import ops
    assert ops.DEFAULT_TIER_COST == {"native": 1.0, "fp8pv": 0.80, "i8pv": 0.59} and ops.TIER_NAMES == ("native", "fp8pv", "i8pv")
    fid = _fid([16.0], [[100.0, 100.0, 1.0]])  # full attention alone, in every tier
    assert _route({"i8pv": fid, "fp8pv": fid, "native": fid}, 0.5) == ([0], [2])
    assert _route({"i8pv": fid, "fp8pv": fid, "native": fid}, 0.5, tier_cost={"i8pv": 0.9, "fp8pv": 0.8, "native": 1.0}) == ([0], [1])


def test_refusals():
    from vorta_amd.patch import routes_from_fidelity_tiers
    fid = _fid(REF, ERR)
    with pytest.raises(ValueError, match="max_flops_share"):
        routes_from_fidelity_tiers({"i8pv": fid, "native": fid}, None, dict(work=(3.0, 2.0, 1.0)), max_flops_share=0.5)
    with pytest.raises(ValueError, match="max_flops_share"):
        routes_from_fidelity_tiers({"i8pv": fid}, 0.5, max_flops_share=0.5)
    for bad in (3, -1, "int4", 1.5, True):
        with pytest.raises(ValueError, match="tier"):
            routes_from_fidelity_tiers({bad: fid}, 0.5)
    with pytest.raises(ValueError, match="distinct"):
        routes_from_fidelity_tiers({"i8pv": fid, 2: fid}, 0.5)
    with pytest.raises(ValueError, match="distinct"):
        routes_from_fidelity_tiers({}, 0.5)
    with pytest.raises(ValueError, match="mapping"):
        routes_from_fidelity_tiers([fid], 0.5)
    for cost in ({"i8pv": 0.0}, {"i8pv": -1.0}, {"i8pv": NAN}, {"i8pv": INF}, {"native": 0.0}, {"i8pv": None}, {"i8pv": "1"}):
        with pytest.raises(ValueError, match="tier_cost"):
            routes_from_fidelity_tiers({"i8pv": fid}, 0.5, tier_cost=cost)
    with pytest.raises(ValueError, match="tier"):
        routes_from_fidelity_tiers({"i8pv": fid}, 0.5, tier_cost={"int4": 1.0})
    # a mapping replaces the entries it names; the others keep the default
    assert routes_from_fidelity_tiers({"i8pv": fid, "native": fid}, 0.75, tier_cost={"native": 0.1})[1].tolist() == [0] * 7
    for bound in (None, -0.5, NAN):
        with pytest.raises(ValueError, match="max_rel_error"):
            routes_from_fidelity_tiers({"i8pv": fid}, bound)
