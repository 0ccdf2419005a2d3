"""GPU: `vorta.patch.measured_routes(model, ...)` / `measured_routes_of(model)` on the hard-routing (Eval) mini models of
tests/_mini_diffusers.py, as tests/test_hip_patch_sampled_expert_fidelity.py builds them (latent (4,6,8), S = 192, 16 / 11 text;
a window of (1,1,1), so that the sliding tile is not full attention in another order).

The check that carries the feature: the output under `measured_routes(model, rule)` is `torch.equal` to the output under
`fixed_routes(model, measured_routes_of(model)[0])` on the same inputs -- equal routes give equal bits through every layer, so
the device lists of every layer are the table the context reports, and the table is what the host rule makes of the records.

The rules come from a measurement of the plain forward, so the table is mixed by construction: layer 0's q, k, v do not depend
on any route, its record under the context is the plain forward's, and the bound is the midpoint between the 2nd and 3rd
smallest per-head minimum sparse error of that layer (two sparse heads there, the others dense); the share is half-way between
the dense layer and the layer with every head on its dearer sparse expert."""
import pytest
import torch

import test_hip_patch as TP
from test_hip_patch_sampled_expert_fidelity import _setup

pytestmark = pytest.mark.gpu
N_ROWS, SEED = 64, 3
_RULES = {}


def _forward(model, inputs, kwargs, seed=None, kw=None):
    x = inputs() if seed is None else inputs(seed)
    return model(**x, return_dict=False, self_attention_kwargs=kw or kwargs())[0]


def _rules(family):
    """(bound, share) of the family's fixture, from the plain forward's record of layer 0 -- measured once"""
    if family not in _RULES:
        from vorta.patch import expert_work, sampled_expert_fidelity, sampled_expert_fidelity_of
        model, inputs, kwargs = _setup(family)
        with torch.no_grad(), sampled_expert_fidelity(model, n_rows=N_ROWS, seed=SEED):
            _forward(model, inputs, kwargs)
        rel = sampled_expert_fidelity_of(model).rel_error().cpu()[0, :, :2]
        best = sorted(rel.min(dim=1).values.tolist())
        assert len(best) >= 3 and best[1] < best[2], best
        work = expert_work(kwargs(), TP.TE if family == "hunyuan" else 0)
        assert max(work[1:]) < work[0], work
        _RULES[family] = ((best[1] + best[2]) / 2, (1 + max(work[1:]) / work[0]) / 2)
    return _RULES[family]


def _host_table(fid, family, rule, kwargs):
    from vorta.patch import routes_from_fidelity
    te = TP.TE if family == "hunyuan" else 0
    return routes_from_fidelity(fid, rule.get("max_rel_error"), kwargs(), te, max_flops_share=rule.get("max_flops_share"))


@pytest.mark.parametrize("mode", ["max_rel_error", "max_flops_share"])
@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_measured_routes_are_the_fixed_routes_of_their_table(family, mode):
    from vorta.patch import fixed_routes, measured_routes, measured_routes_of
    from vorta_amd import ops
    from vorta_amd.patch._engine import context_of
    bound, share = _rules(family)
    rule = {mode: bound if mode == "max_rel_error" else share}
    model, inputs, kwargs = _setup(family)
    ctx = context_of(model)
    L, H = len(ctx.plan), ctx.plan.heads
    with pytest.raises(RuntimeError, match="measured_routes_of"):
        measured_routes_of(model)
    with torch.no_grad():
        plain = _forward(model, inputs, kwargs)
        with measured_routes(model, n_rows=N_ROWS, seed=SEED, **rule):
            out = _forward(model, inputs, kwargs)
            kw = kwargs()
            kw.pop("tau_sparse")
            assert torch.equal(_forward(model, inputs, kwargs, kw=kw), out), "tau_sparse is not consulted under measured_routes"
            experts, fid = measured_routes_of(model)
    assert ctx.measured_routes is None
    assert experts.is_cuda and experts.dtype == torch.int32 and experts.shape == (L, H)
    assert isinstance(fid, ops.ExpertFidelity) and fid.sq_err.shape == (L, H, 3) and fid.n == N_ROWS * 128
    assert bool(torch.isnan(fid.sq_err[..., 2]).all()) and bool(torch.isfinite(fid.sq_err[..., :2]).all())
    table = experts.cpu().long()
    print(f"{family} {rule}: rel_error\n{fid.rel_error().cpu()[..., :2]}\ntable\n{table}")
    assert len(set(table.flatten().tolist())) >= 2, f"a table of one expert proves nothing: {table}"
    if mode == "max_rel_error":
        assert sum(int(e) != 0 for e in table[0]) == 2  # layer 0: the two heads under the bound
    assert torch.equal(_host_table(fid, family, rule, kwargs), table), "the device routes are the host rule's"
    assert torch.equal(measured_routes_of(model)[0], experts)  # (still on record outside the context)
    with torch.no_grad(), fixed_routes(model, experts):
        fixed = _forward(model, inputs, kwargs)
    assert torch.equal(out, fixed), "equal routes give equal bits through every layer"
    assert not torch.equal(out, plain)  # (the routers' routes are other routes)
    with torch.no_grad():
        assert torch.equal(_forward(model, inputs, kwargs), plain), "outside the context nothing changes"


@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_refresh_every_two_measures_every_other_forward(family, monkeypatch):
    import vorta_amd.routed as rt
    from vorta.patch import fixed_routes, measured_routes, measured_routes_of
    from vorta_amd.patch._engine import context_of
    bound, _ = _rules(family)
    model, inputs, kwargs = _setup(family)
    L = len(context_of(model).plan)
    calls, real = [], rt.sampled_expert_fidelity
    monkeypatch.setattr(rt, "sampled_expert_fidelity", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    with torch.no_grad(), measured_routes(model, max_rel_error=bound, n_rows=N_ROWS, seed=SEED, refresh_every=2):
        _forward(model, inputs, kwargs)
        assert len(calls) == L
        first = measured_routes_of(model)[0].clone()
        second_out = _forward(model, inputs, kwargs, seed=11)       # other inputs: no measurement, the first forward's lists
        assert len(calls) == L
        assert torch.equal(measured_routes_of(model)[0], first)
        third_out = _forward(model, inputs, kwargs, seed=11)        # measures again, on these inputs
        assert len(calls) == 2 * L
        third = measured_routes_of(model)[0].clone()
    assert len(set(first.flatten().tolist())) >= 2
    with torch.no_grad():
        with fixed_routes(model, first):
            assert torch.equal(_forward(model, inputs, kwargs, seed=11), second_out), "the second forward launches the first's table"
        with fixed_routes(model, third):
            assert torch.equal(_forward(model, inputs, kwargs, seed=11), third_out)
    print(f"{family}: first table {first.tolist()}, third {third.tolist()}")
    assert len(calls) == 2 * L


def test_routed_fidelity_inside_reports_the_measured_routes():
    from vorta.patch import measured_routes, measured_routes_of, routed_fidelity, routed_fidelity_of
    bound, _ = _rules("wan")
    model, inputs, kwargs = _setup("wan")
    with torch.no_grad():
        with measured_routes(model, max_rel_error=bound, n_rows=N_ROWS, seed=SEED):
            alone = _forward(model, inputs, kwargs)
            with routed_fidelity(model, n_rows=N_ROWS, seed=SEED, heads="all"):
                out = _forward(model, inputs, kwargs)
        experts, fid = measured_routes_of(model)
    rf = routed_fidelity_of(model)
    assert torch.equal(out, alone)
    assert torch.equal(rf.expert, experts), "the record reports the routes as launched: the measured ones"
    # a sparse head's measured error is the column the route was chosen by, to the two reductions' chains of roundings
    from vorta_amd import _C
    tol = (_C.fidelity_chain(N_ROWS) + _C.sampled_fidelity_chain(N_ROWS) + 4) * 2.0 ** -24
    got, rel, sparse = rf.rel_error().cpu(), fid.rel_error().cpu(), 0
    for layer, row in enumerate(experts.tolist()):
        for h, e in enumerate(row):
            if e:
                sparse += 1
                want = float(rel[layer, h, e - 1])
                assert abs(float(got[layer, h]) - want) <= tol * want and want <= bound, (layer, h, e, float(got[layer, h]), want)
    assert sparse > 0


def test_refusals_by_message(monkeypatch):
    from vorta.patch import fixed_routes, measured_routes, routed_fidelity, sampled_expert_fidelity
    from vorta_amd.patch._engine import context_of
    from vorta_amd.ulysses import SP_STATE
    model, _, _ = _setup("wan")
    ctx = context_of(model)
    L, H = len(ctx.plan), ctx.plan.heads
    table = torch.zeros((L, H), dtype=torch.int64)

    def refused(exc, match, *contexts):
        with pytest.raises(exc, match=match):
            stack = []
            try:
                for make in contexts:
                    cm = make()
                    cm.__enter__()
                    stack.append(cm)
            finally:
                for cm in reversed(stack):
                    cm.__exit__(None, None, None)

    by_bound = lambda **kw: (lambda: measured_routes(model, max_rel_error=0.1, **kw))  # noqa: E731
    refused(ValueError, "measured_routes: the model was not patched", lambda: measured_routes(torch.nn.Linear(2, 2), max_rel_error=0.1))
    refused(ValueError, "exactly one of max_rel_error and max_flops_share", lambda: measured_routes(model))
    refused(ValueError, "exactly one of max_rel_error and max_flops_share",
            lambda: measured_routes(model, max_rel_error=0.1, max_flops_share=0.5))
    refused(ValueError, "measured_routes inside fixed_routes", lambda: fixed_routes(model, table), by_bound())
    refused(ValueError, "fixed_routes inside measured_routes", by_bound(), lambda: fixed_routes(model, table))
    refused(ValueError, "measured_routes inside sampled_expert_fidelity", lambda: sampled_expert_fidelity(model), by_bound())
    refused(ValueError, "sampled_expert_fidelity inside measured_routes", by_bound(), lambda: sampled_expert_fidelity(model))
    refused(ValueError, "measured_routes inside measured_routes", by_bound(), by_bound())
    refused(ValueError, "share one sample", lambda: routed_fidelity(model, n_rows=32, seed=0), by_bound(n_rows=64))
    refused(ValueError, "share one sample", by_bound(n_rows=64, seed=1), lambda: routed_fidelity(model, n_rows=64, seed=0))
    refused(ValueError, "refresh_every", by_bound(refresh_every=0))
    monkeypatch.setattr(SP_STATE, "_enabled", True)  # (the flag alone: the context refuses before anything is launched)
    refused(NotImplementedError, "measured_routes: routing by a measurement does not run under sequence parallelism", by_bound())
    monkeypatch.undo()
    assert ctx.measured_routes is None and ctx.fixed_routes is None and ctx.measure_experts is None and ctx.measure_routed is None


def test_more_refusals_of_the_context(monkeypatch):
    """no sampled row (every error would read 0 and every head meet any bound); soft-mixture (Train) processors; a forward
    between two measurements that finds no stored routes raises instead of falling back to the routers"""
    from vorta.patch import measured_routes
    from vorta_amd.patch._engine import context_of
    from vorta_amd.routed import RouteRule, route_by_fidelity
    model, inputs, kwargs = _setup("wan")
    ctx = context_of(model)
    with pytest.raises(ValueError, match="measured_routes: n_rows=0"):
        with measured_routes(model, max_rel_error=0.1, n_rows=0):
            pass
    with pytest.raises(ValueError, match="RouteRule"):
        RouteRule("max_rel_error", 0.1, n_rows=0)
    with pytest.raises(ValueError, match="at least one sampled row"):
        route_by_fidelity(None, None, None, None, model="wan", rows=0, max_rel_error=0.1)
    monkeypatch.setattr(ctx, "needs_tau", False)  # what apply_vorta_transformer(train_router=True) leaves: Train processors
    with pytest.raises(ValueError, match="soft-mixture"):
        with measured_routes(model, max_rel_error=0.1):
            pass
    monkeypatch.undo()
    bound, _ = _rules("wan")
    with torch.no_grad(), measured_routes(model, max_rel_error=bound, n_rows=N_ROWS, seed=SEED, refresh_every=2):
        _forward(model, inputs, kwargs)
        ctx.measured_routes.filed.pop(1)
        with pytest.raises(RuntimeError, match="layer 1 has no measured routes on record"):
            _forward(model, inputs, kwargs)
    assert ctx.measured_routes is None and ctx.current is None


def _eval_call(family):
    """one direct call of the family's Eval processor on an attention module of tests/_mini_diffusers.py: (call, kwargs)"""
    import inspect

    import _mini_diffusers as M
    from test_hip_patch_sampled_expert_fidelity import _kwargs
    from _util import dev
    from vorta_amd.attention import hunyuan as hy, wan
    torch.manual_seed(17)
    bf, S, T, te = torch.bfloat16, TP.S, TP.T, TP.TE
    cls = wan.WanAttnProcessorTripleEval if family == "wan" else hy.HunyuanVideoFlashAttnProcessorTripleEval
    accepted = set(inspect.signature(cls.__call__).parameters) - {"tau_sparse"}  # (as the patch's BoundProcessor filters)
    kw = {k: v for k, v in _kwargs(family).items() if k in accepted}
    hidden = torch.randn((1, S, M.INNER), device=dev()).to(bf)
    score = torch.full((1, M.H, 3), 1.0 / 3, device=dev())
    if family == "wan":
        attn = M.MiniAttention(M.INNER, norm="across_heads").to(dev()).to(bf)
        proc = wan.WanAttnProcessorTripleEval()
        return lambda **more: proc(attn, hidden, None, None, None, tau_sparse=0.3, routing_score=score, **kw, **more)
    attn = M.MiniAttention(M.INNER, added_kv=True).to(dev()).to(bf)
    proc = hy.HunyuanVideoFlashAttnProcessorTripleEval()
    enc = torch.randn((1, T, M.INNER), device=dev()).to(bf)
    ang = torch.rand((S, 64), device=dev()) * 6.28
    rope = (ang.cos().repeat_interleave(2, dim=1).contiguous(), ang.sin().repeat_interleave(2, dim=1).contiguous())
    mask = torch.zeros((1, 1, 1, S + T), dtype=torch.bool, device=dev())
    mask[..., :S + te] = True
    return lambda **more: proc(attn, hidden, enc, mask, rope, routing_score=score, tau_sparse=0.3, **kw, **more)


@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_eval_processors_take_a_rule_and_refuse_it_under_sequence_parallelism(family, monkeypatch):
    """a direct call: with a rule the sink receives (expert_ids, lists, counts, fid) and routing_score / tau_sparse are not
    consulted; with the sequence-parallel flag set the processor refuses by name, before anything is exchanged (the flag alone
    is set: a group of one, whose shards are the whole tensors); the Train processors take no rule"""
    import inspect

    from vorta_amd import ops
    from vorta_amd.attention import hunyuan as hy, wan
    from vorta_amd.routed import RouteRule
    from vorta_amd.ulysses import SP_STATE
    for cls in (hy.HunyuanVideoFlashAttnProcessorTripleTrain, wan.WanAttnProcessorTripleTrain):
        assert "route_rule" not in inspect.signature(cls.__call__).parameters
    call = _eval_call(family)
    rule = RouteRule("max_flops_share", 0.8, n_rows=N_ROWS, seed=SEED)
    sink = []
    with torch.no_grad():
        plain, routed = call(), call(route_rule=rule, route_sink=sink)
    first = lambda y: y[0] if isinstance(y, tuple) else y  # noqa: E731
    assert first(routed).shape == first(plain).shape and bool(torch.isfinite(first(routed).float()).all())
    assert len(sink) == 1 and len(sink[0]) == 4
    ids, lists, counts, fid = sink[0]
    assert ids.dtype == torch.int32 and lists.shape == (3, ids.numel()) and counts.shape == (3,) and isinstance(fid, ops.ExpertFidelity)
    assert int(counts.sum()) == ids.numel() and len(set(ids.tolist())) >= 2
    monkeypatch.setattr(SP_STATE, "_enabled", True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="route_rule: routing by a measured error bound"):
        call(route_rule=rule, route_sink=[])
    monkeypatch.undo()
    with torch.no_grad():
        assert torch.equal(first(call()), first(plain))
