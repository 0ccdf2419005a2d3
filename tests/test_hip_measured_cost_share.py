"""GPU: routing (precision, expert) pairs by a COST budget -- `routed.route_by_fidelity(max_cost_share=...)` and
`vorta.patch.measured_routes(model, max_cost_share=...)` with `measured_levels_of`, against the host rule
`vorta.patch.routes_within_cost_share` on CPU copies of the records the calls return.

Operator: the inputs, geometry and rows of tests/test_hip_measured_precision.py (five heads, latent (9,18,16), 128 sampled rows)
under the process precisions "native" (ONE tier: the only new path through the launchers), "i8pv" and "auto8".  Patch layer: the
mini models of tests/test_hip_patch_measured_routes.py.  The tables must equal the host rule's with `==`; what is launched must
equal, bit for bit, a replay of the tables through `fixed_routes(model, experts, precisions=...)`."""
import pytest
import torch

from test_hip_measured_precision import NAMES, _cpu, _operator_case, precision  # noqa: F401  (`precision` is a fixture)
from test_hip_patch_measured_routes import _eval_call, _forward
from test_hip_patch_sampled_expert_fidelity import _setup
import test_hip_patch as TP

pytestmark = pytest.mark.gpu
N_PATCH, SEED = 64, 3
SHARES = (0.3, 0.45, 0.7)


@pytest.mark.parametrize("process", ["native", "i8pv", "auto8"])
def test_operator_routes_by_the_budget_and_launches_the_tiers(process, precision):
    from vorta.patch import routes_within_cost_share
    from vorta_amd import ops
    from vorta_amd.routed import (TIERS_OF_PRECISION, HeadRouting, TierRoutes, route_by_fidelity, routed_attention,
                                  routed_attention_tiers)
    precision(process)
    c = _operator_case()
    q, k, v, geom, rows, dev = (c[x] for x in ("q", "k", "v", "geom", "rows", "dev"))
    tiers, H = TIERS_OF_PRECISION[process], q.shape[1]
    route_by_fidelity(q, k, v, geom, model="wan", rows=rows, max_cost_share=SHARES[0])  # (warm)
    torch.cuda.synchronize()
    levels = []
    for share in SHARES:
        torch.cuda.set_sync_debug_mode("error")  # any host <-> device synchronisation in here raises
        try:
            routes = route_by_fidelity(q, k, v, geom, model="wan", rows=rows, max_cost_share=share)
            out = routed_attention_tiers(q, k, v, routes.routings, geom, model="wan", operands=routes.operands)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert isinstance(routes, TierRoutes) and tuple(routes.routings) == tiers and tuple(routes.fids) == tiers
        assert routes.level.shape == (1,) and routes.level.dtype == torch.float32 and routes.level.is_cuda
        want = routes_within_cost_share({t: _cpu(routes.fids[t]) for t in tiers}, share, geom, 0)
        experts, tier_ids, level = routes.expert_ids.tolist(), routes.tier_ids.tolist(), float(routes.level)
        print(f"{process} share {share}: experts {experts}, tiers {tier_ids}, level {level}, host cost share {float(want.cost_share)}")
        assert (experts, tier_ids) == (want.experts.tolist(), want.tiers.tolist()), "the device tables are the host rule's"
        assert level == float(want.level)
        counts = routes.counts.tolist()
        for i, t in enumerate(tiers):
            for e in range(3):
                heads = [h for h in range(H) if tier_ids[h] == ops.tier_id(t) and experts[h] == e]
                assert counts[i][e] == len(heads) and routes.lists[i, e, :len(heads)].tolist() == heads, (t, e)
        # every head's output is what routed_attention(fp8=its tier) writes for it under its expert, from host-count lists
        by_experts = HeadRouting.from_expert_ids(experts, dev)
        for t in tiers:
            whole = routed_attention(q, k, v, by_experts, geom, model="wan", fp8=False if t == "native" else t)
            for h in range(H):
                if tier_ids[h] == ops.tier_id(t):
                    assert torch.equal(out[0, h], whole[0, h]), (h, experts[h], t)
        levels.append(level)
    assert levels[0] >= levels[1] >= levels[2], f"a growing share never raises the level: {levels}"
    assert levels[0] > 0, "the smallest share does spend on sparse or 8-bit launches"
    with pytest.raises(ValueError, match="exactly one of"):
        route_by_fidelity(q, k, v, geom, model="wan", rows=rows, max_cost_share=0.5, max_rel_error=0.1)
    with pytest.raises(ValueError, match="exactly one of"):
        route_by_fidelity(q, k, v, geom, model="wan", rows=rows, max_cost_share=0.5, max_flops_share=0.5)
    with pytest.raises(ValueError, match="exactly one of"):
        route_by_fidelity(q, k, v, geom, model="wan", rows=rows)
    with pytest.raises(ValueError, match="max_cost_share"):
        route_by_fidelity(q, k, v, geom, model="wan", rows=rows, max_cost_share=0.0)


def test_operator_graph_replay_under_the_one_native_tier(precision):
    """no host read: a measuring call and its launches captured with static q, k, v; a replay on other inputs gives the tables,
    the level and the output of the eager calls"""
    from vorta_amd.routed import route_by_fidelity, routed_attention_tiers
    precision("native")
    c = _operator_case()
    geom, rows = c["geom"], c["rows"]
    first = (c["q"], c["k"], c["v"])
    second = (c["q"].flip(1).contiguous(), c["k"].flip(1).contiguous(), c["v"].flip(1).contiguous())  # the heads in reverse order
    kw = dict(model="wan", rows=rows, max_cost_share=SHARES[1])
    q, k, v = (x.clone() for x in first)
    out = torch.empty_like(q)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        routes = route_by_fidelity(q, k, v, geom, **kw)
        routed_attention_tiers(q, k, v, routes.routings, geom, model="wan", out=out, operands=routes.operands)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        routes = route_by_fidelity(q, k, v, geom, **kw)
        routed_attention_tiers(q, k, v, routes.routings, geom, model="wan", out=out, operands=routes.operands)
    assert tuple(routes.routings) == ("native",)
    tables = []
    for inputs in (second, first):
        for dst, src in zip((q, k, v), inputs):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        eager = route_by_fidelity(*inputs, geom, **kw)
        want = routed_attention_tiers(*inputs, eager.routings, geom, model="wan", operands=eager.operands)
        assert torch.equal(routes.expert_ids, eager.expert_ids) and torch.equal(routes.tier_ids, eager.tier_ids)
        assert torch.equal(routes.counts, eager.counts) and torch.equal(routes.level, eager.level) and torch.equal(out, want)
        tables.append(routes.expert_ids.tolist())
    print(f"replayed tables {tables}")
    assert tables[0] == list(reversed(tables[1])) and len(set(tables[1])) >= 2


def _host_layer(data, share, kwargs, family, tier_cost=None):
    from vorta.patch import routes_within_cost_share
    te = TP.TE if family == "hunyuan" else 0
    return routes_within_cost_share({t: _cpu(data["fids"][t]) for t in data["tiers"]}, share, kwargs(), te, tier_cost=tier_cost)


@pytest.mark.parametrize("process", ["native", "i8pv", "auto8"])
@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_measured_cost_share_is_the_host_rule_and_the_fixed_routes_of_its_tables(family, process, precision):
    from vorta.patch import fixed_routes, measured_levels_of, measured_precisions_of, measured_routes, measured_routes_of
    from vorta_amd.patch._engine import context_of
    from vorta_amd.routed import TIERS_OF_PRECISION
    precision(process)
    model, inputs, kwargs = _setup(family)
    ctx = context_of(model)
    L, H = len(ctx.plan), ctx.plan.heads
    share = 0.45
    with pytest.raises(RuntimeError, match="measured_levels_of"):
        measured_levels_of(model)
    with torch.no_grad():
        plain = _forward(model, inputs, kwargs)
        with measured_routes(model, max_cost_share=share, n_rows=N_PATCH, seed=SEED):
            out = _forward(model, inputs, kwargs)
            experts, _ = measured_routes_of(model)
            tiers, levels = measured_precisions_of(model), measured_levels_of(model)
            filed = {layer: entries[0][4] for layer, entries in ctx.measured_routes.filed.items()}
    assert ctx.measured_routes is None
    assert levels.is_cuda and levels.dtype == torch.float32 and levels.shape == (L,)
    assert experts.shape == (L, H) == tiers.shape and tiers.dtype == torch.int32
    print(f"{family} {process} share {share}: experts\n{experts.cpu()}\ntiers\n{tiers.cpu()}\nlevels {levels.tolist()}")
    for i, layer in enumerate(sorted(filed)):
        data = filed[layer]
        assert data["tiers"] == TIERS_OF_PRECISION[process]
        want = _host_layer(data, share, kwargs, family)
        assert experts[i].tolist() == want.experts.tolist() and tiers[i].tolist() == want.tiers.tolist(), f"layer {layer}"
        assert float(levels[i]) == float(want.level), f"layer {layer}"
    assert float(levels.max()) > 0, "the budget does spend on sparse or 8-bit launches"
    assert torch.equal(measured_levels_of(model), levels)  # (still on record outside the context)
    with torch.no_grad(), fixed_routes(model, experts, precisions=tiers):
        fixed = _forward(model, inputs, kwargs)
    assert torch.equal(out, fixed), "equal routes in equal tiers give equal bits through every layer"
    with torch.no_grad():
        assert torch.equal(_forward(model, inputs, kwargs), plain), "outside the context nothing changes"
        with measured_routes(model, max_rel_error=0.1, n_rows=N_PATCH, seed=SEED):
            _forward(model, inputs, kwargs)
        with pytest.raises(RuntimeError, match="not routed by max_cost_share"):
            measured_levels_of(model)


def test_tier_cost_and_refresh_every_work_as_for_the_bound(precision, monkeypatch):
    import vorta_amd.routed as rt
    from vorta.patch import fixed_routes, measured_levels_of, measured_precisions_of, measured_routes, measured_routes_of
    from vorta_amd.patch._engine import context_of
    precision("i8pv")
    model, inputs, kwargs = _setup("wan")
    ctx = context_of(model)
    L = len(ctx.plan)
    cost = {"i8pv": 0.25}
    calls, real = [], rt.sampled_expert_fidelity
    monkeypatch.setattr(rt, "sampled_expert_fidelity", lambda *a, **kw: (calls.append(kw.get("precision")), real(*a, **kw))[1])
    with torch.no_grad(), measured_routes(model, max_cost_share=0.45, n_rows=N_PATCH, seed=SEED, tier_cost=cost, refresh_every=2):
        _forward(model, inputs, kwargs)
        assert calls == [None, "i8pv"] * L  # one measurement per tier and layer
        first = (measured_routes_of(model)[0].clone(), measured_precisions_of(model).clone(), measured_levels_of(model).clone())
        data = ctx.measured_routes.filed[sorted(ctx.measured_routes.filed)[0]][0][4]
        second_out = _forward(model, inputs, kwargs, seed=11)  # other inputs: no measurement, the first forward's lists
        assert len(calls) == 2 * L and torch.equal(measured_levels_of(model), first[2])
    want = _host_layer(data, 0.45, kwargs, "wan", tier_cost=cost)
    assert first[0][0].tolist() == want.experts.tolist() and first[1][0].tolist() == want.tiers.tolist()
    assert float(first[2][0]) == float(want.level)
    with torch.no_grad(), fixed_routes(model, first[0], precisions=first[1]):
        assert torch.equal(_forward(model, inputs, kwargs, seed=11), second_out), "the second forward launches the first's tables"


@pytest.mark.parametrize("process", ["native", "i8pv"])
def test_repair_above_below_the_level_brings_the_heads_over_it_back_dense(process, precision):
    from vorta.patch import measured_levels_of, measured_routes, measured_routes_of, repaired_routes_of
    precision(process)
    model, inputs, kwargs = _setup("wan")
    share = 0.3
    with torch.no_grad(), measured_routes(model, max_cost_share=share, n_rows=N_PATCH, seed=SEED):
        _forward(model, inputs, kwargs)
        level0 = float(measured_levels_of(model)[0])
        before = measured_routes_of(model)[0][0].tolist()
    assert level0 > 0, "layer 0's budget buys an error: choose a smaller share"
    bound = level0 / 2  # layer 0's q, k, v depend on no route: the head that sits AT the level is launched far over the bound
    with torch.no_grad(), measured_routes(model, max_cost_share=share, n_rows=N_PATCH, seed=SEED, repair_above=bound):
        _forward(model, inputs, kwargs)
        rel, state, experts, tiers = (x.cpu() for x in repaired_routes_of(model))
    print(f"{process}: level {level0}, bound {bound}\nrel {rel.tolist()}\nstate {state.tolist()}\nexperts {experts.tolist()}")
    assert 2 in state[0].tolist(), "a head of layer 0 is over half its level"
    checked = state > 0
    assert bool((state[checked & ~(rel <= bound)] == 2).all()) and bool((state[checked & (rel <= bound)] == 1).all())
    assert bool((experts[state == 2] == 0).all()) and bool((tiers[state == 2] == 0).all()), "repaired heads are dense, native"
    kept = [h for h, s in enumerate(state[0].tolist()) if s != 2]
    assert [experts[0, h].item() for h in kept] == [before[h] for h in kept]


def test_eval_processors_file_the_level_and_the_rule_names_its_tiers(precision, monkeypatch):
    from vorta_amd.routed import ROUTE_RULE_MODES, RouteRule
    from vorta_amd.ulysses import SP_STATE
    assert ROUTE_RULE_MODES == ("max_rel_error", "max_flops_share", "max_cost_share")
    precision("native")
    rule = RouteRule("max_cost_share", 0.45, n_rows=N_PATCH, seed=SEED, tier_cost={"native": 1.0})
    assert rule.tiers() == ("native",)
    assert RouteRule("max_rel_error", 0.1, covers_precision=True).tiers() is None  # (the bound under "native": experts alone)
    call, sink = _eval_call("wan"), []
    with torch.no_grad():
        routed = call(route_rule=rule, route_sink=sink)
    assert len(sink) == 1 and len(sink[0]) == 5
    ids, lists, counts, fid, data = sink[0]
    H = ids.numel()
    assert lists.shape == (1, 3, H) and counts.shape == (1, 3) and int(counts.sum()) == H
    assert data["tiers"] == ("native",) and data["level"].shape == (1,) and not bool(data["tier_ids"].any())
    with torch.no_grad():  # the stored lists launch the same bits
        from vorta_amd.routed import HeadRouting
        first = lambda y: y[0] if isinstance(y, tuple) else y  # noqa: E731
        stored = {"native": HeadRouting.from_device(lists[0], counts[0])}
        assert torch.equal(first(call(tier_routing=stored)), first(routed))
    precision("auto8")
    assert rule.tiers() == ("i8pv", "fp8pv", "native")
    monkeypatch.setattr(SP_STATE, "_enabled", True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="route_rule: routing by a measured error bound"):
        call(route_rule=rule, route_sink=[])
    monkeypatch.undo()
    with pytest.raises(ValueError, match="covers_precision goes with max_rel_error"):
        RouteRule("max_flops_share", 0.5, covers_precision=True)


def test_refusals_by_name(precision, monkeypatch):
    from vorta.patch import measured_routes
    from vorta_amd.patch._engine import context_of
    from vorta_amd.ulysses import SP_STATE
    precision("i8pv")
    model, _, _ = _setup("wan")

    def refused(exc, match, make):
        with pytest.raises(exc, match=match):
            with make():
                pass

    one = "exactly one of max_rel_error and max_flops_share and max_cost_share"
    refused(ValueError, one, lambda: measured_routes(model))
    refused(ValueError, one, lambda: measured_routes(model, max_cost_share=0.5, max_rel_error=0.1))
    refused(ValueError, one, lambda: measured_routes(model, max_cost_share=0.5, max_flops_share=0.5))
    refused(ValueError, one, lambda: measured_routes(model, max_rel_error=0.1, max_flops_share=0.5, max_cost_share=0.5))
    refused(ValueError, "max_cost_share=0.0", lambda: measured_routes(model, max_cost_share=0.0))
    refused(ValueError, "max_cost_share=nan", lambda: measured_routes(model, max_cost_share=float("nan")))
    refused(ValueError, "tier_cost", lambda: measured_routes(model, max_cost_share=0.5, tier_cost={"i8pv": 0.0}))
    refused(ValueError, "covers_precision with max_flops_share", lambda: measured_routes(model, max_flops_share=0.5, covers_precision=True))
    monkeypatch.setattr(SP_STATE, "_enabled", True)
    refused(NotImplementedError, "does not run under sequence parallelism", lambda: measured_routes(model, max_cost_share=0.5))
    monkeypatch.undo()
    with measured_routes(model, max_cost_share=0.5, repair_above=0.1):  # (no covers_precision needed: it is implied)
        assert context_of(model).measured_routes.rule.covers_precision
    assert context_of(model).measured_routes is None
