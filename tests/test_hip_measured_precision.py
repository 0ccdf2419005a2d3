"""GPU: routing every head's PRECISION by the measured error bound -- `routed.route_by_fidelity(tiers=...)`,
`routed.routed_attention_tiers`, and `vorta.patch.measured_routes(..., covers_precision=True)` with
`measured_precisions_of` / `fixed_routes(model, table, precisions=...)`.

Operator: the inputs of tests/test_hip_i8.py `_auto8_case` -- heads from white, student_t3, smooth, student_t3, outlier_w,
latent (9,18,16), S = 2592, Wan -- on 128 sampled rows, tiers (i8pv, fp8pv, native).  The bound is the midpoint between the
2nd and 3rd smallest per-head "i8pv" full-attention error of a first measurement; that no candidate's rel lies within 10 % of
it is asserted as a condition on the inputs (the full-size launch cuts its keys otherwise than the measurement does: another
realisation of the e4m3 rounding of P, a few per cent of the 8-bit error), in a test of its own; the seeds are chosen for it.

Patch layer: the mini models of tests/test_hip_patch_measured_routes.py under "i8pv" and "auto8"."""
import pytest
import torch

from test_hip_i8 import _auto8_case
from test_hip_patch_measured_routes import _eval_call, _forward
from test_hip_patch_sampled_expert_fidelity import _setup

pytestmark = pytest.mark.gpu

FAMS = ["white", "student_t3", "smooth", "student_t3", "outlier_w"]
TIERS = ("i8pv", "fp8pv", "native")
N_ROWS = 128
# seeds of `_auto8_case` and of `sample_rows`, chosen for the condition on the inputs below (see that test)
INPUT_SEED, ROWS_SEED = 90, 1
NAMES = ("sq_ref", "max_ref", "sq_err", "max_err", "range_ref")
_OP = {}


@pytest.fixture()
def precision():
    """sets the process precision for a test and puts back what was there"""
    import vorta_amd.routed as rt
    before = rt.DEFAULT_FP8
    yield rt.set_attention_precision
    rt.DEFAULT_FP8 = before


def _cpu(fid):
    return fid._replace(**{name: getattr(fid, name).cpu() for name in NAMES})


def _operator_case():
    """q, k, v, the geometry, the rows, the first measurement per tier and the bound -- once"""
    if not _OP:
        from vorta_amd.routed import RoutedGeometry, sample_rows, sampled_expert_fidelity
        dev = torch.device("cuda")
        latent, q, k, v = _auto8_case(dev, FAMS, seed=INPUT_SEED)
        geom = RoutedGeometry(latent, tile=(3, 6, 8), window=(3, 3, 3), group=(3, 3, 2), rate=0.5, device=dev)
        rows = sample_rows(geom.S, N_ROWS, ROWS_SEED, dev)
        first = {t: sampled_expert_fidelity(q, k, v, geom, model="wan", rows=rows, precision=None if t == "native" else t)
                 for t in TIERS}
        rel = {t: f.rel_error().cpu() for t, f in first.items()}
        full_i8 = sorted(rel["i8pv"][:, 2].tolist())
        bound = (full_i8[1] + full_i8[2]) / 2
        print(f"rel_error per tier (coreset, sliding, full):\n" + "\n".join(f"{t}: {rel[t].tolist()}" for t in TIERS)
              + f"\ni8pv full-attention errors sorted {full_i8} -> bound {bound}")
        _OP.update(q=q, k=k, v=v, geom=geom, rows=rows, first=first, rel=rel, bound=bound, dev=dev)
    return _OP


def test_operator_inputs_keep_every_candidate_ten_percent_from_the_bound():
    """A condition on the INPUTS, not on the code: no candidate's rel within 10 % of the bound, so that the few per cent between
    a candidate and its full-size launch cannot carry a head across it.  Most seeds miss it: the 2nd and 3rd smallest "i8pv"
    full-attention errors are the white-noise and the outlier-weight head's, 0.040 - 0.047 and 0.043 - 0.055 (the smooth head
    reads 0.009 - 0.011, the two Student-t heads 0.05 - 0.13), and a midpoint keeps 10 % from both its neighbours only where they
    differ by more than 22 %.  Measured on an MI355X over input seeds 0..159 x row seeds 0..2: two pairs meet it, (90, 1) with
    the nearest candidate at 0.122 of the bound (errors 0.0098, 0.0422, 0.0543, 0.080, 0.080), used here, and (109, 2) at 0.106;
    `_auto8_case`'s default seed 5 with row seed 0 lies at 0.028."""
    c = _operator_case()
    bound = c["bound"]
    cands = torch.cat([c["rel"][t].flatten() for t in TIERS])  # (native's column 2 is NaN: it is the reference)
    cands = cands[~torch.isnan(cands)]
    near = cands[((cands - bound).abs() <= 0.1 * bound)]
    assert near.numel() == 0, f"candidates within 10 % of the bound {bound}: {near.tolist()} -- choose other seeds"


def test_operator_routes_tiers_by_the_bound_and_launches_them():
    from vorta_amd.patch import routes_from_fidelity_tiers
    from vorta_amd.routed import HeadRouting, TierRoutes, route_by_fidelity, routed_attention, routed_attention_tiers
    from vorta_amd import ops
    c = _operator_case()
    q, k, v, geom, rows, bound, dev = (c[x] for x in ("q", "k", "v", "geom", "rows", "bound", "dev"))
    H = len(FAMS)
    kw = dict(model="wan", rows=rows, max_rel_error=bound, tiers=TIERS)
    route_by_fidelity(q, k, v, geom, **kw)  # (warm)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # any host <-> device synchronisation in here raises
    try:
        routes = route_by_fidelity(q, k, v, geom, **kw)
        out = routed_attention_tiers(q, k, v, routes.routings, geom, model="wan", operands=routes.operands)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert isinstance(routes, TierRoutes) and tuple(routes.routings) == TIERS and set(routes.operands) == {"i8pv", "fp8pv"}
    assert routes.operands["fp8pv"].v is routes.operands["i8pv"].v  # V was converted once
    for t in TIERS:  # the records are the first measurement's, bit for bit
        for name in NAMES:
            a, b = getattr(routes.fids[t], name), getattr(c["first"][t], name)
            assert torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) and torch.equal(torch.isnan(a), torch.isnan(b)), (t, name)
    experts, tiers = routes.expert_ids.tolist(), routes.tier_ids.tolist()
    print(f"bound {bound}: experts {experts}, tiers {tiers} ({[ops.TIER_NAMES[t] for t in tiers]})")
    assert len(set(tiers)) >= 2, f"a table of one tier proves nothing: {tiers}"
    want_e, want_t = routes_from_fidelity_tiers({t: _cpu(routes.fids[t]) for t in TIERS}, bound, geom, 0)
    assert (experts, tiers) == (want_e.tolist(), want_t.tolist()), "the device tables are the host rule's"
    counts = routes.counts.tolist()
    for i, t in enumerate(TIERS):
        for e in range(3):
            heads = [h for h in range(H) if tiers[h] == ops.tier_id(t) and experts[h] == e]
            assert counts[i][e] == len(heads) and routes.lists[i, e, :len(heads)].tolist() == heads, (t, e)
    # every head's output is what routed_attention(fp8=its tier) writes for it under the chosen expert
    by_experts = HeadRouting.from_expert_ids(experts, dev)
    whole = {t: routed_attention(q, k, v, by_experts, geom, model="wan", fp8=False if t == "native" else t) for t in TIERS}
    for h in range(H):
        assert torch.equal(out[0, h], whole[ops.TIER_NAMES[tiers[h]]][0, h]), (h, experts[h], tiers[h])
    # converting its own operands changes no bit
    assert torch.equal(routed_attention_tiers(q, k, v, routes.routings, geom, model="wan"), out)
    # what was LAUNCHED, on the same rows, against dense attention in the input dtype: within the bound, head by head
    sink = []
    again = routed_attention_tiers(q, k, v, routes.routings, geom, model="wan", operands=routes.operands, fidelity=sink,
                                   fidelity_rows=rows, fidelity_heads="all")
    assert torch.equal(again, out) and len(sink) == 1 and sink[0].expert.tolist() == experts
    launched = sink[0].rel_error().cpu()
    cand = torch.stack([torch.zeros(()) if (tiers[h] == 0 and experts[h] == 0) else
                        routes.fids[ops.TIER_NAMES[tiers[h]]].rel_error().cpu()[h, 2 if experts[h] == 0 else experts[h] - 1]
                        for h in range(H)])
    print(f"launched rel_error {launched.tolist()}\ncandidate rel_error {cand.tolist()}\n"
          f"launched / candidate {[float(a / b) if b > 0 else None for a, b in zip(launched, cand)]}")
    assert bool(torch.isfinite(launched).all()) and bool((launched <= bound).all()), (launched.tolist(), bound)
    with pytest.raises(ValueError, match="max_flops_share has no form over precision tiers"):
        route_by_fidelity(q, k, v, geom, model="wan", rows=rows, max_flops_share=0.5, tiers=TIERS)
    with pytest.raises(ValueError, match="does not apply"):
        routed_attention_tiers(q, k, v, routes.routings, geom, model="wan", fp8="i8pv")


def test_operator_graph_replay_on_other_inputs():
    """no host read: captured with static q, k, v; a replay on other inputs gives the tables and the output of the eager calls"""
    from vorta_amd.routed import route_by_fidelity, routed_attention_tiers
    c = _operator_case()
    geom, rows, bound = c["geom"], c["rows"], c["bound"]
    first = (c["q"], c["k"], c["v"])
    second = (c["q"].flip(1).contiguous(), c["k"].flip(1).contiguous(), c["v"].flip(1).contiguous())  # the heads in reverse order
    kw = dict(model="wan", rows=rows, max_rel_error=bound, tiers=TIERS)
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
    tables = []
    for inputs in (second, first):
        for dst, src in zip((q, k, v), inputs):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        eager = route_by_fidelity(*inputs, geom, **kw)
        want = routed_attention_tiers(*inputs, eager.routings, geom, model="wan", operands=eager.operands)
        assert torch.equal(routes.expert_ids, eager.expert_ids) and torch.equal(routes.tier_ids, eager.tier_ids)
        assert torch.equal(routes.counts, eager.counts) and torch.equal(out, want)
        tables.append((routes.expert_ids.tolist(), routes.tier_ids.tolist()))
    print(f"replayed tables {tables}")
    assert tables[0] == tuple(list(reversed(x)) for x in tables[1]) and len(set(tables[1][1])) >= 2


# ---- the patch layer ---------------------------------------------------------------------------------------------------------

N_PATCH, SEED = 64, 3


def _patch_bound(model, inputs, kwargs):
    """the midpoint between the 2nd and 3rd smallest per-head "i8pv" full-attention error of layer 0 (whose q, k, v depend on no
    route), from a first measuring forward under the current process precision"""
    from vorta.patch import measured_routes
    from vorta_amd.patch._engine import context_of
    with torch.no_grad(), measured_routes(model, max_rel_error=0.0, n_rows=N_PATCH, seed=SEED, covers_precision=True):
        _forward(model, inputs, kwargs)
    data = context_of(model).latest_measured_routes.filed[0][0][4]
    full = sorted(data["fids"]["i8pv"].rel_error().cpu()[:, 2].tolist())
    assert full[1] < full[2], full
    return (full[1] + full[2]) / 2


@pytest.mark.parametrize("process", ["i8pv", "auto8"])
@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_measured_precisions_are_the_fixed_routes_of_their_tables(family, process, precision):
    from vorta.patch import fixed_routes, measured_precisions_of, measured_routes, measured_routes_of
    from vorta_amd.patch._engine import context_of
    from vorta_amd.routed import TIERS_OF_PRECISION
    from vorta_amd import ops
    precision(process)
    model, inputs, kwargs = _setup(family)
    ctx = context_of(model)
    L, H = len(ctx.plan), ctx.plan.heads
    bound = _patch_bound(model, inputs, kwargs)
    with torch.no_grad():
        plain = _forward(model, inputs, kwargs)
        with measured_routes(model, max_rel_error=bound, n_rows=N_PATCH, seed=SEED):  # without the flag: experts alone
            _forward(model, inputs, kwargs)
            assert not bool(measured_precisions_of(model).any()), "routes over experts alone read tier 0"
        with measured_routes(model, max_rel_error=bound, n_rows=N_PATCH, seed=SEED, covers_precision=True):
            out = _forward(model, inputs, kwargs)
            experts, fid = measured_routes_of(model)
            tiers = measured_precisions_of(model)
    assert tiers.is_cuda and tiers.dtype == torch.int32 and tiers.shape == (L, H) == experts.shape
    assert isinstance(fid, ops.ExpertFidelity) and fid.sq_err.shape == (L, H, 3)  # (the native tier's records: the method's error)
    offered = {ops.tier_id(t) for t in TIERS_OF_PRECISION[process]}
    print(f"{family} {process} bound {bound}: experts\n{experts.cpu()}\ntiers\n{tiers.cpu()}")
    assert set(tiers.flatten().tolist()) <= offered and len(set(tiers.flatten().tolist())) >= 2, tiers.tolist()
    assert torch.equal(measured_precisions_of(model), tiers)  # (still on record outside the context)
    with torch.no_grad(), fixed_routes(model, experts, precisions=tiers):
        fixed = _forward(model, inputs, kwargs)
    assert torch.equal(out, fixed), "equal routes in equal tiers give equal bits through every layer"
    assert not torch.equal(out, plain)  # (the routers' routes in the process precision are other launches)
    with torch.no_grad():
        assert torch.equal(_forward(model, inputs, kwargs), plain), "outside the context nothing changes"


@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_refresh_every_two_launches_the_stored_tiers(family, precision, monkeypatch):
    import vorta_amd.routed as rt
    from vorta.patch import fixed_routes, measured_precisions_of, measured_routes, measured_routes_of
    from vorta_amd.patch._engine import context_of
    precision("i8pv")
    model, inputs, kwargs = _setup(family)
    L = len(context_of(model).plan)
    bound = _patch_bound(model, inputs, kwargs)
    calls, real = [], rt.sampled_expert_fidelity
    monkeypatch.setattr(rt, "sampled_expert_fidelity", lambda *a, **kw: (calls.append(kw.get("precision")), real(*a, **kw))[1])
    with torch.no_grad(), measured_routes(model, max_rel_error=bound, n_rows=N_PATCH, seed=SEED, refresh_every=2,
                                          covers_precision=True):
        _forward(model, inputs, kwargs)
        assert calls == [None, "i8pv"] * L  # one measurement per tier and layer
        first = (measured_routes_of(model)[0].clone(), measured_precisions_of(model).clone())
        second_out = _forward(model, inputs, kwargs, seed=11)  # other inputs: no measurement, the first forward's lists
        assert len(calls) == 2 * L
        assert torch.equal(measured_precisions_of(model), first[1])
    assert len(set(first[1].flatten().tolist())) >= 2
    with torch.no_grad(), fixed_routes(model, first[0], precisions=first[1]):
        assert torch.equal(_forward(model, inputs, kwargs, seed=11), second_out), "the second forward launches the first's tiers"


@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_under_native_the_flag_changes_no_bit(family, precision):
    from vorta.patch import measured_precisions_of, measured_routes, measured_routes_of
    from test_hip_patch_measured_routes import _rules
    precision("native")
    bound, _ = _rules(family)
    model, inputs, kwargs = _setup(family)
    with torch.no_grad():
        with measured_routes(model, max_rel_error=bound, n_rows=N_PATCH, seed=SEED):
            want, table = _forward(model, inputs, kwargs), measured_routes_of(model)[0].clone()
        with measured_routes(model, max_rel_error=bound, n_rows=N_PATCH, seed=SEED, covers_precision=True):
            got = _forward(model, inputs, kwargs)
            assert torch.equal(measured_routes_of(model)[0], table) and not bool(measured_precisions_of(model).any())
    assert torch.equal(got, want) and len(set(table.flatten().tolist())) >= 2


@pytest.mark.parametrize("family", ["hunyuan", "wan"])
def test_eval_processors_file_a_five_tuple_and_refuse_under_sequence_parallelism(family, precision, monkeypatch):
    from vorta_amd import ops
    from vorta_amd.routed import RouteRule
    from vorta_amd.ulysses import SP_STATE
    precision("auto8")
    call = _eval_call(family)
    rule = RouteRule("max_rel_error", 0.05, n_rows=N_PATCH, seed=SEED, covers_precision=True)
    sink = []
    with torch.no_grad():
        plain, routed = call(), call(route_rule=rule, route_sink=sink)
    first = lambda y: y[0] if isinstance(y, tuple) else y  # noqa: E731
    assert first(routed).shape == first(plain).shape and bool(torch.isfinite(first(routed).float()).all())
    assert len(sink) == 1 and len(sink[0]) == 5
    ids, lists, counts, fid, data = sink[0]
    H = ids.numel()
    assert lists.shape == (3, 3, H) and counts.shape == (3, 3) and int(counts.sum()) == H and isinstance(fid, ops.ExpertFidelity)
    assert data["tiers"] == ("i8pv", "fp8pv", "native") and data["tier_ids"].shape == (H,) and set(data["fids"]) == set(data["tiers"])
    with torch.no_grad():  # the stored lists launch the same bits
        from vorta_amd.routed import HeadRouting
        stored = {t: HeadRouting.from_device(lists[i], counts[i]) for i, t in enumerate(data["tiers"])}
        assert torch.equal(first(call(tier_routing=stored)), first(routed))
    monkeypatch.setattr(SP_STATE, "_enabled", True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="route_rule: routing by a measured error bound"):
        call(route_rule=rule, route_sink=[])
    with torch.no_grad(), pytest.raises(NotImplementedError, match="tier_routing"):
        call(tier_routing=stored)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="covers_precision goes with max_rel_error"):
        RouteRule("max_flops_share", 0.5, covers_precision=True)


def test_refusals_by_name(precision):
    from vorta.patch import fixed_routes, measured_routes
    from vorta_amd.patch._engine import context_of
    precision("i8pv")
    model, _, _ = _setup("wan")
    ctx = context_of(model)
    L, H = len(ctx.plan), ctx.plan.heads
    table = torch.zeros((L, H), dtype=torch.int64)

    def refused(exc, match, make):
        with pytest.raises(exc, match=match):
            with make():
                pass

    refused(ValueError, "covers_precision with max_flops_share", lambda: measured_routes(model, max_flops_share=0.5, covers_precision=True))
    refused(ValueError, "tier_cost goes with covers_precision", lambda: measured_routes(model, max_rel_error=0.1, tier_cost={"i8pv": 0.5}))
    refused(ValueError, "tier_cost", lambda: measured_routes(model, max_rel_error=0.1, covers_precision=True, tier_cost={"i8pv": 0.0}))
    refused(ValueError, "precision tier ids are 0", lambda: fixed_routes(model, table, precisions=table + 3))
    refused(ValueError, "precision tier ids are 0", lambda: fixed_routes(model, table, precisions=table - 1))
    refused(ValueError, "integer tier table of shape", lambda: fixed_routes(model, table, precisions=table[:, :1]))
    refused(ValueError, "does not offer", lambda: fixed_routes(model, table, precisions=table + 1))  # fp8pv under "i8pv"
    precision("native")
    refused(ValueError, "does not offer", lambda: fixed_routes(model, table, precisions=table + 2))
    with fixed_routes(model, table, precisions=table):
        assert ctx.fixed_precisions == [[0] * H] * L
    assert ctx.fixed_routes is None and ctx.fixed_precisions is None and ctx.measured_routes is None
