"""GPU: `measured_routes(model, ..., repair_above=b)`, `fixed_routes(model, table, ..., repair_above=b)` and
`repaired_routes_of(model)` on the hard-routing (Eval) mini models of tests/test_hip_patch_measured_routes.py.

What is expected comes from TODAY's paths and the host rule.  A forward that launches stored routes on other inputs is
measured by `routed_fidelity(model)` (the same sample): inside a context with `repair_above` that record reports the rows as
they were BEFORE the repair, so `vorta.patch.repair_routes` on it, with the routes as launched, names the heads the forward must
have repaired -- layer by layer, on that forward's own q, k, v.  Layer 0's q, k, v depend on no route: its record is also
compared with today's forward by the same table, bit for bit.  And equal routes give equal bits: the repaired forward's output
is `torch.equal` to today's `fixed_routes` forward by the table AFTER the repair.

The bound b.  The first forward measures on inputs A and launches routes whose launched error is at most a_max; the second
launches them on inputs B (seed 11), where the largest launched error of a stored sparse head is b_max.  b = (a_max + b_max) / 2,
from a preliminary run of today's paths: with a_max < b < b_max the first forward repairs nothing and the second repairs at
least one head -- in the first layer that holds a head over b, whose inputs are the preliminary run's.  That b_max > a_max is a
condition on the inputs, asserted where b is made.

`refresh_every`.  With `refresh_every=2` the context's third forward MEASURES again (forwards 0, 2, 4, ...): it writes fresh
tables.  That a later forward launches the repaired heads dense without a second repair is therefore shown with
`refresh_every=3`, whose third forward launches the stored -- repaired -- tables."""
import pytest
import torch

from test_hip_patch_measured_routes import _eval_call, _forward, _rules
from test_hip_patch_sampled_expert_fidelity import _setup

pytestmark = pytest.mark.gpu
N_ROWS, SEED, SEED_B = 64, 3, 11
_PRE = {}


@pytest.fixture()
def precision():
    """sets the process precision for a test and puts back what was there"""
    import vorta_amd.routed as rt
    before = rt.DEFAULT_FP8
    yield rt.set_attention_precision
    rt.DEFAULT_FP8 = before


def _same(a, b) -> bool:
    a, b = a.cpu(), b.cpu()
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0.0, 1e30, -1e30), b.nan_to_num(0.0, 1e30, -1e30))


def _preliminary(family):
    """today's paths, once per family: the measuring forward on A and the stored-route forward on B under
    `measured_routes(refresh_every=2)`, both measured by `routed_fidelity`; the table, the records, the outputs and b"""
    if family not in _PRE:
        from vorta.patch import measured_routes, measured_routes_of, routed_fidelity, routed_fidelity_of
        bound, _ = _rules(family)
        model, inputs, kwargs = _setup(family)
        with torch.no_grad(), routed_fidelity(model, n_rows=N_ROWS, seed=SEED, heads="sparse"), \
                measured_routes(model, max_rel_error=bound, n_rows=N_ROWS, seed=SEED, refresh_every=2):
            out_a = _forward(model, inputs, kwargs)
            rec_a, table = routed_fidelity_of(model), measured_routes_of(model)[0].clone()
            out_b = _forward(model, inputs, kwargs, seed=SEED_B)
            rec_b = routed_fidelity_of(model)
        sparse = table.cpu() != 0
        rel_a, rel_b = rec_a.rel_error().cpu(), rec_b.rel_error().cpu()
        a_max, b_max = float(rel_a[sparse].max()), float(rel_b[sparse].max())
        print(f"{family}: table\n{table.cpu()}\nlaunched rel on A\n{rel_a}\non B\n{rel_b}\na_max {a_max} b_max {b_max}")
        assert b_max > a_max * 1.02, f"{family}: inputs B do not break a stored route further than A's own ({a_max}, {b_max})"
        _PRE[family] = dict(bound=bound, table=table, rec_b=rec_b, out_a=out_a, out_b=out_b, b=(a_max + b_max) / 2)
    return _PRE[family]


def _host_rule(experts, tiers, n_tiers, exact, rec, b):
    """`repair_routes` layer by layer on a stacked record: (state, experts after, caller's tier index after), each (L, H)"""
    from vorta.patch import repair_routes
    rows = [repair_routes(experts[l], None if tiers is None else tiers[l], n_tiers, exact, rec.sq_ref[l].cpu(), rec.sq_err[l].cpu(), b)
            for l in range(experts.shape[0])]
    return (torch.stack([r.state_of_head for r in rows]), torch.stack([r.expert_of_head for r in rows]),
            torch.stack([r.tier_of_head for r in rows]), torch.stack([r.rel for r in rows]))


def _read(model):
    from vorta.patch import repaired_routes_of
    return [x.clone() for x in repaired_routes_of(model)]


@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_measured_routes_repair_a_stored_route_that_breaks_the_bound(family):
    from vorta.patch import fixed_routes, measured_routes, measured_routes_of, routed_fidelity, routed_fidelity_of
    from vorta_amd.patch._engine import context_of
    pre = _preliminary(family)
    b, table = pre["b"], pre["table"]
    model, inputs, kwargs = _setup(family)
    ctx = context_of(model)
    L, H = len(ctx.plan), ctx.plan.heads
    with torch.no_grad(), routed_fidelity(model, n_rows=N_ROWS, seed=SEED, heads="sparse"), \
            measured_routes(model, max_rel_error=pre["bound"], n_rows=N_ROWS, seed=SEED, refresh_every=2, repair_above=b):
        out1 = _forward(model, inputs, kwargs)
        rel1, state1, experts1, tiers1 = _read(model)
        out2 = _forward(model, inputs, kwargs, seed=SEED_B)
        rec2 = routed_fidelity_of(model)
        rel2, state2, experts2, tiers2 = _read(model)
        stored = measured_routes_of(model)[0].clone()
        _forward(model, inputs, kwargs, seed=SEED_B)  # forward 2 of the context measures again: fresh tables
        rel3, state3, experts3, _ = _read(model)
        rec3 = routed_fidelity_of(model)
    assert ctx.route_repair is None and ctx.measured_routes is None
    for t, dtype in ((rel1, torch.float32), (state1, torch.int32), (experts1, torch.int32), (tiers1, torch.int32)):
        assert t.is_cuda and t.dtype == dtype and t.shape == (L, H)
    # the measuring forward: verified, nothing over b, the bits of today's forward
    assert not bool((state1 == 2).any()) and torch.equal(experts1, table) and not bool(tiers1.any())
    assert torch.equal(state1 != 0, table != 0)  # the sparse heads of the native tier are the checked ones
    assert torch.equal(out1, pre["out_a"])
    # the stored-route forward on B: exactly the host rule's heads, by its own record
    assert torch.equal(rec2.expert, table), "the record reports the routes as launched, before the repair"
    state, experts, _, rel = _host_rule(table.cpu().long(), None, 1, 0, rec2, b)
    print(f"{family}: b {b} state\n{state2.cpu()}\nrel as checked\n{rel2.cpu()}")
    assert torch.equal(state2.cpu().long(), state) and torch.equal(experts2.cpu().long(), experts) and _same(rel2, rel)
    assert int((state == 2).sum()) >= 1 and int((state == 1).sum()) >= 1, state
    assert not bool(tiers2.any()) and torch.equal(stored, experts2), "the stored tables hold the repair"
    for name in ("sq_ref", "sq_err", "max_err"):  # layer 0 depends on no route: today's record of the same launches
        assert _same(getattr(rec2, name)[0], getattr(pre["rec_b"], name)[0]), name
    assert not torch.equal(out2, pre["out_b"])
    with torch.no_grad(), fixed_routes(model, experts2):
        assert torch.equal(_forward(model, inputs, kwargs, seed=SEED_B), out2), "equal routes give equal bits through every layer"
    # the third forward measured: its tables are fresh, and its repairs are the host rule's on its own record
    state, experts, _, _ = _host_rule(rec3.expert.cpu().long(), None, 1, 0, rec3, b)
    assert torch.equal(state3.cpu().long(), state) and torch.equal(experts3.cpu().long(), experts)
    # refresh_every=3: the third forward launches the repaired tables -- dense, without a second repair
    with torch.no_grad(), measured_routes(model, max_rel_error=pre["bound"], n_rows=N_ROWS, seed=SEED, refresh_every=3,
                                          repair_above=b):
        _forward(model, inputs, kwargs)
        second = _forward(model, inputs, kwargs, seed=SEED_B)
        _, s2, e2, _ = _read(model)
        third = _forward(model, inputs, kwargs, seed=SEED_B)
        _, s3, e3, _ = _read(model)
    assert torch.equal(s2, state2) and torch.equal(e2, experts2) and torch.equal(second, out2)
    assert not bool((s3 == 2).any()) and torch.equal(s3, torch.where(s2 == 2, torch.zeros_like(s2), s2)) and torch.equal(e3, e2)
    assert torch.equal(third, second)
    with torch.no_grad():  # outside the contexts, and with None, every forward keeps its bits
        plain = _forward(model, inputs, kwargs)
        with measured_routes(model, max_rel_error=pre["bound"], n_rows=N_ROWS, seed=SEED, repair_above=None):
            assert ctx.route_repair is None
            assert torch.equal(_forward(model, inputs, kwargs), pre["out_a"])
        assert torch.equal(_forward(model, inputs, kwargs), plain)


@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_fixed_routes_repair_a_reused_table_and_reset_on_entry(family):
    from vorta.patch import fixed_routes, routed_fidelity, routed_fidelity_of
    from vorta_amd.patch._engine import context_of
    pre = _preliminary(family)
    b, table = pre["b"], pre["table"]
    model, inputs, kwargs = _setup(family)
    ctx = context_of(model)
    with torch.no_grad():
        with fixed_routes(model, table):
            today = _forward(model, inputs, kwargs, seed=SEED_B)
        with fixed_routes(model, table, repair_above=None):
            assert ctx.route_repair is None and torch.equal(_forward(model, inputs, kwargs, seed=SEED_B), today)
        with fixed_routes(model, table, repair_above=b, n_rows=N_ROWS, seed=SEED):
            with routed_fidelity(model, n_rows=N_ROWS, seed=SEED):
                out = _forward(model, inputs, kwargs, seed=SEED_B)
            rec = routed_fidelity_of(model)
            rel, state, experts, tiers = _read(model)
            again = _forward(model, inputs, kwargs, seed=SEED_B)  # the repairs persist: launched dense, no second repair
            _, state_again, experts_again, _ = _read(model)
        with fixed_routes(model, table, repair_above=b, n_rows=N_ROWS, seed=SEED):  # entered again: from the table
            _forward(model, inputs, kwargs, seed=SEED_B)
            _, state_reset, experts_reset, _ = _read(model)
    assert torch.equal(today, pre["out_b"])
    want_state, want_experts, _, want_rel = _host_rule(table.cpu().long(), None, 1, 0, rec, b)
    assert torch.equal(rec.expert, table)
    assert torch.equal(state.cpu().long(), want_state) and torch.equal(experts.cpu().long(), want_experts) and _same(rel, want_rel)
    assert int((want_state == 2).sum()) >= 1 and int((want_state == 1).sum()) >= 1 and not bool(tiers.any())
    assert not bool((state_again == 2).any()) and torch.equal(experts_again, experts) and torch.equal(again, out)
    assert torch.equal(state_reset, state) and torch.equal(experts_reset, experts)
    with torch.no_grad(), fixed_routes(model, experts):
        assert torch.equal(_forward(model, inputs, kwargs, seed=SEED_B), out)
    assert ctx.route_repair is None and ctx.fixed_routes is None


@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_fixed_routes_with_precisions_repair_into_the_native_tier(family, precision):
    """every head in "i8pv": an 8-bit tier verifies EVERY head, full attention included, and a repaired head moves to
    (expert 0, native); b is the middle of layer 0's launched errors in today's forward by the same tables"""
    from vorta.patch import fixed_routes, routed_fidelity, routed_fidelity_of
    from vorta_amd.patch._engine import context_of
    precision("i8pv")
    pre = _preliminary(family)
    table = pre["table"]
    model, inputs, kwargs = _setup(family)
    L, H = len(context_of(model).plan), context_of(model).plan.heads
    i8 = torch.full((L, H), 2, dtype=torch.int64)
    with torch.no_grad():
        with fixed_routes(model, table, precisions=i8), routed_fidelity(model, n_rows=N_ROWS, seed=SEED, heads="all"):
            _forward(model, inputs, kwargs, seed=SEED_B)
        rec_today = routed_fidelity_of(model)
        layer0 = sorted(rec_today.rel_error().cpu()[0].tolist())
        assert layer0[H // 2 - 1] < layer0[H // 2], layer0
        b = (layer0[H // 2 - 1] + layer0[H // 2]) / 2
        with fixed_routes(model, table, precisions=i8, repair_above=b, n_rows=N_ROWS, seed=SEED):
            with routed_fidelity(model, n_rows=N_ROWS, seed=SEED):
                out = _forward(model, inputs, kwargs, seed=SEED_B)
            rec = routed_fidelity_of(model)
            rel, state, experts, tiers = _read(model)
            again = _forward(model, inputs, kwargs, seed=SEED_B)
            _, state_again, experts_again, tiers_again = _read(model)
    # tiers in launch order (i8pv, native): every head starts at index 0; the exact tier is index 1
    zeros = torch.zeros((L, H), dtype=torch.int64)
    want_state, want_experts, want_index, want_rel = _host_rule(table.cpu().long(), zeros, 2, 1, rec, b)
    print(f"{family} i8pv: b {b} state\n{state.cpu()}\nrel as checked\n{rel.cpu()}")
    assert torch.equal(state.cpu().long(), want_state) and torch.equal(experts.cpu().long(), want_experts) and _same(rel, want_rel)
    assert torch.equal(tiers.cpu().long(), torch.where(want_index == 1, 0, 2)), "global tier ids after the repair"
    assert bool((want_state != 0).all())  # every head of an 8-bit tier is checked
    assert int((want_state[0] == 2).sum()) == H - H // 2 and int((want_state[0] == 1).sum()) == H // 2, want_state
    for name in ("sq_ref", "sq_err", "max_err"):
        assert _same(getattr(rec, name)[0], getattr(rec_today, name)[0]), name
    assert not bool((state_again == 2).any()) and torch.equal(experts_again, experts) and torch.equal(tiers_again, tiers)
    assert torch.equal(again, out)
    with torch.no_grad(), fixed_routes(model, experts, precisions=tiers):
        assert torch.equal(_forward(model, inputs, kwargs, seed=SEED_B), out), "equal routes in equal tiers give equal bits"


def test_refusals_are_by_name(precision, monkeypatch):
    from vorta.patch import fixed_routes, measured_routes, repaired_routes_of, routed_fidelity
    from vorta_amd.patch._engine import context_of
    from vorta_amd.routed import RouteRule
    from vorta_amd.ulysses import SP_STATE
    model, inputs, kwargs = _setup("wan")
    ctx = context_of(model)
    L, H = len(ctx.plan), ctx.plan.heads
    table = torch.zeros((L, H), dtype=torch.int64)

    def refused(exc, match, make):
        with pytest.raises(exc, match=match):
            with make():
                pass

    with pytest.raises(RuntimeError, match="repaired_routes_of"):
        repaired_routes_of(model)
    for bad in (-0.25, float("nan")):
        refused(ValueError, "measured_routes: repair_above", lambda: measured_routes(model, max_rel_error=0.1, repair_above=bad))
        refused(ValueError, "fixed_routes: repair_above", lambda: fixed_routes(model, table, repair_above=bad))
        with pytest.raises(ValueError, match="repair_above"):
            RouteRule("max_rel_error", 0.1, repair_above=bad)
    assert RouteRule("max_flops_share", 0.5).repair_above is None and RouteRule("max_flops_share", 0.5, 64, 0, False, None, 0.2).repair_above == 0.2
    precision("i8pv")
    refused(ValueError, "measured_routes: repair_above under the 8-bit process precision 'i8pv' needs tier routes",
            lambda: measured_routes(model, max_rel_error=0.1, repair_above=0.1))
    refused(ValueError, "fixed_routes: repair_above under the 8-bit process precision 'i8pv' needs tier routes",
            lambda: fixed_routes(model, table, repair_above=0.1))
    with measured_routes(model, max_rel_error=0.1, covers_precision=True, repair_above=0.1):
        assert ctx.route_repair is not None and ctx.measured_routes.rule.repair_above == pytest.approx(0.1)
    with fixed_routes(model, table, precisions=table, repair_above=0.1):
        assert ctx.route_repair.bound == pytest.approx(0.1)
    precision("native")
    with measured_routes(model, max_flops_share=0.5, repair_above=0.1, n_rows=N_ROWS, seed=SEED):  # with both rules
        refused(ValueError, "share one sample", lambda: routed_fidelity(model, n_rows=N_ROWS + 1, seed=SEED))
    with fixed_routes(model, table, repair_above=0.1, n_rows=N_ROWS, seed=SEED):
        refused(ValueError, "share one sample", lambda: routed_fidelity(model, n_rows=N_ROWS, seed=SEED + 1))
    with routed_fidelity(model, n_rows=N_ROWS, seed=SEED):
        refused(ValueError, "share one sample", lambda: fixed_routes(model, table, repair_above=0.1, n_rows=N_ROWS, seed=SEED + 1))
    assert ctx.route_repair is None and ctx.fixed_routes is None and ctx.measured_routes is None
    # sequence parallelism: the contexts, and the processors by the name of the keyword
    monkeypatch.setattr(SP_STATE, "_enabled", True)
    refused(NotImplementedError, "measured_routes", lambda: measured_routes(model, max_rel_error=0.1, repair_above=0.1))
    refused(NotImplementedError, "fixed_routes", lambda: fixed_routes(model, table, repair_above=0.1))
    for family in ("hunyuan", "wan"):
        with torch.no_grad(), pytest.raises(NotImplementedError, match="repair_above: verifying and repairing"):
            _eval_call(family)(repair_above=0.1, repair_sink=[])
    monkeypatch.undo()


@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_eval_processors_repair_a_device_head_routing(family):
    """a direct call with a device `head_routing` (its expert ids derived from its lists): the sink receives the call's
    record; a bound no head can break leaves the output its bits; a bound of 0 re-runs every sparse head, rewrites the
    routing's lists in place, and gives the all-dense call's bits"""
    import _mini_diffusers as M
    import test_hip_patch as TP
    from _util import dev
    from vorta_amd.routed import HeadRouting, RepairRecord, sample_rows
    call = _eval_call(family)
    rows = sample_rows(TP.S, N_ROWS, SEED, dev())
    first = lambda y: y[0] if isinstance(y, tuple) else y  # noqa: E731
    experts = [(1, 2, 0)[h % 3] for h in range(M.H)]

    def device_routing(ids):
        host = HeadRouting.from_expert_ids(ids, dev())
        return HeadRouting.from_device(host.lists, torch.tensor(host.counts_host, dtype=torch.int32).to(dev()))

    sink, zero = [], []
    with torch.no_grad():
        plain = first(call(head_routing=device_routing(experts)))
        dense = first(call(head_routing=device_routing([0] * M.H)))
        kept = first(call(head_routing=device_routing(experts), repair_above=float("inf"), repair_sink=sink, fidelity_rows=rows))
        routing = device_routing(experts)
        every = first(call(head_routing=routing, repair_above=0.0, repair_sink=zero, fidelity_rows=rows))
    assert len(sink) == 1 and isinstance(sink[0], RepairRecord) and int(sink[0].repair_count) == 0
    assert sink[0].state_of_head.tolist() == [0 if e == 0 else 1 for e in experts]
    assert torch.equal(kept, plain)
    assert zero[0].state_of_head.tolist() == [0 if e == 0 else 2 for e in experts]
    assert zero[0].repair_list[:int(zero[0].repair_count)].tolist() == [h for h, e in enumerate(experts) if e != 0]
    assert routing.counts_dev.tolist() == [M.H, 0, 0] and routing.lists[0].tolist() == list(range(M.H))
    assert torch.equal(every, dense) and not torch.equal(every, plain)
