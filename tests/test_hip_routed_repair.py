"""GPU: `routed.routed_attention_repaired` -- launch, verify on sampled rows, decide on the device (vorta_route_repair), re-run
the heads over the bound dense in the input dtype, all in one call without a host read.

Inputs: tests/test_hip_measured_precision.py's -- `_auto8_case(dev, FAMS, seed=90)` (Wan, latent (9,18,16), S = 2592, 5 heads from
five input families), `sample_rows(S, 128, 1)`, tile (3,6,8), window (3,3,3), coreset window (3,3,2) at rate 0.5.  What is
expected comes from TODAY's calls on the same tensors: the record of `routed_attention_tiers(..., fidelity=)` /
`routed_attention(..., fidelity=)`, the host rule `vorta.patch.repair_routes` on that record, and `routed_attention(fp8=False)`
under expert 0 for what a repaired head must hold.  The bound is the midpoint between the 2nd and 3rd smallest rel of that
record, so some heads are repaired and some kept (asserted on its own).  Everything compared is compared for EQUALITY."""
import pytest
import torch

from test_hip_i8 import _auto8_case

pytestmark = pytest.mark.gpu

FAMS = ["white", "student_t3", "smooth", "student_t3", "outlier_w"]
H = len(FAMS)
N_ROWS, INPUT_SEED, ROWS_SEED = 128, 90, 1
T_HY, TE_HY = 8, 5  # Hunyuan's text rows as tests/_sp_soft_mixture.py has them: 8, of which 5 are valid
SPARSE = [1, 2, 1, 2, 0]  # case 2: sparse experts, one head on full attention (not checked)
NAMES = ("sq_ref", "max_ref", "sq_err", "max_err", "range_ref")
_C = {}


def _i32(x, dev):
    return torch.tensor(x, dtype=torch.int32).to(dev)


def _tier_tables(dev):
    """device tables of tiers (i8pv, native) with every head on full attention in i8pv"""
    from vorta_amd.routed import RepairableRoutes
    lists = torch.zeros((2, 3, H), dtype=torch.int32)
    lists[0, 0] = torch.arange(H, dtype=torch.int32)
    return RepairableRoutes(("i8pv", "native"), _i32([0] * H, dev), _i32([0] * H, dev), lists.to(dev),
                            _i32([[H, 0, 0], [0, 0, 0]], dev))


def _single_tables(dev, experts=SPARSE):
    """(HeadRouting.from_device, expert_ids) of `experts` under the single native tier"""
    from vorta_amd.routed import HeadRouting
    host = HeadRouting.from_expert_ids(experts, dev)
    return HeadRouting.from_device(host.lists, _i32(host.counts_host, dev)), _i32(experts, dev)


def _cpu(fid):
    return {name: getattr(fid, name).cpu() for name in NAMES}


def _same_record(a, b) -> bool:
    a, b = _cpu(a), _cpu(b)
    return all(torch.equal(a[n].isnan(), b[n].isnan()) and torch.equal(a[n].nan_to_num(0.0), b[n].nan_to_num(0.0)) for n in NAMES)


def _bound_of(rel, checked):
    """the midpoint between the 2nd and 3rd smallest rel among the checked heads"""
    r = sorted(float(rel[h]) for h in checked)
    return (r[1] + r[2]) / 2


def _case():
    """the inputs, today's calls on them and what the host rule makes of their records -- computed once, left unchanged"""
    if _C:
        return _C
    from vorta_amd.patch import repair_routes
    from vorta_amd.routed import HeadRouting, RoutedGeometry, routed_attention, routed_attention_tiers, sample_rows
    dev = torch.device("cuda")
    latent, q, k, v = _auto8_case(dev, FAMS, seed=INPUT_SEED)
    geom = RoutedGeometry(latent, tile=(3, 6, 8), window=(3, 3, 3), group=(3, 3, 2), rate=0.5, device=dev)
    rows = sample_rows(geom.S, N_ROWS, ROWS_SEED, dev)
    # case 1: today's tier launch with its fidelity sink, and full attention in the input dtype under expert 0
    tables = _tier_tables(dev)
    sink = []
    today = routed_attention_tiers(q, k, v, tables.routings, geom, model="wan", out=torch.zeros_like(q), fidelity=sink,
                                   fidelity_rows=rows, fidelity_heads="all")
    dense = routed_attention(q, k, v, HeadRouting.from_expert_ids([0] * H, dev), geom, model="wan", out=torch.zeros_like(q), fp8=False)
    rel = sink[0].rel_error().cpu()
    bound = _bound_of(rel, range(H))
    want = repair_routes([0] * H, [0] * H, 2, 1, sink[0].sq_ref.cpu(), sink[0].sq_err.cpu(), bound)
    _C["wan"] = dict(today=today, dense=dense, record=sink[0], rel=rel, bound=bound, want=want)
    # case 2: the Hunyuan form -- the same video rows and 8 text rows, 5 valid; one native tier, sparse experts
    g = torch.Generator(device=dev).manual_seed(INPUT_SEED)
    qh, kh, vh = (torch.cat([x, torch.randn((1, H, T_HY, 128), generator=g, device=dev).to(x.dtype)], 2).contiguous()
                  for x in (q, k, v))
    hy = dict(model="hunyuan", text_len=T_HY, text_valid=TE_HY)
    routing, _ = _single_tables(dev)
    sink = []
    today = routed_attention(qh, kh, vh, routing, geom, out=torch.zeros_like(qh), fp8=False, fidelity=sink, fidelity_rows=rows,
                             fidelity_heads="sparse", **hy)
    dense = routed_attention(qh, kh, vh, HeadRouting.from_expert_ids([0] * H, dev), geom, out=torch.zeros_like(qh), fp8=False, **hy)
    rel = sink[0].rel_error().cpu()
    checked = [h for h in range(H) if SPARSE[h] != 0]
    bound = _bound_of(rel, checked)
    want = repair_routes(SPARSE, None, 1, 0, sink[0].sq_ref.cpu(), sink[0].sq_err.cpu(), bound)
    _C["hunyuan"] = dict(q=qh, k=kh, v=vh, kw=hy, today=today, dense=dense, record=sink[0], rel=rel, bound=bound, want=want)
    _C.update(q=q, k=k, v=v, geom=geom, rows=rows, dev=dev)
    print(f"case 1 rel {_C['wan']['rel'].tolist()} bound {_C['wan']['bound']}; case 2 rel {rel.tolist()} bound {bound}")
    return _C


def _check_tables(routes, want, case):
    assert routes.expert_ids.tolist() == want.expert_of_head.tolist(), case
    if routes.tier_index is not None:
        assert routes.tier_index.tolist() == want.tier_of_head.tolist(), case
    assert routes.counts.tolist() == want.counts.tolist(), case
    for t in range(want.counts.shape[0]):
        for e in range(3):
            n = int(want.counts[t, e])
            assert routes.lists[t, e, :n].tolist() == want.lists[t, e, :n].tolist(), (case, t, e)


def _check_record(rec, want, case):
    n = want.repair_count
    assert int(rec.repair_count) == n and rec.repair_list[:n].tolist() == want.repair_list[:n].tolist(), case
    assert rec.state_of_head.tolist() == want.state_of_head.tolist(), case
    got, ref = rec.rel.cpu(), want.rel
    assert torch.equal(got.isnan(), ref.isnan()) and torch.equal(got.nan_to_num(0.0), ref.nan_to_num(0.0)), case


def test_the_inputs_have_heads_on_both_sides_of_the_bound():
    """A condition on the INPUTS: in both cases at least one head is repaired and at least one checked head is kept, and the
    2nd and 3rd smallest rel differ, so the midpoint separates them."""
    c = _case()
    for name in ("wan", "hunyuan"):
        state = c[name]["want"].state_of_head.tolist()
        assert state.count(2) >= 1 and state.count(1) >= 1, (name, state, c[name]["rel"].tolist(), c[name]["bound"])
    assert c["hunyuan"]["want"].state_of_head[4] == 0  # the full-attention head of the native tier is not checked


def test_tiers_every_head_full_in_i8pv_is_verified_decided_and_repaired():
    from vorta_amd.routed import routed_attention_repaired
    c = _case()
    w = c["wan"]
    tables = _tier_tables(c["dev"])
    out, rec = routed_attention_repaired(c["q"], c["k"], c["v"], tables, c["geom"], repair_above=w["bound"], rows=c["rows"],
                                         model="wan", out=torch.zeros_like(c["q"]))
    torch.cuda.synchronize()
    assert _same_record(rec.fidelity, w["record"])  # the same launches: the verification record is today's, bit for bit
    assert torch.equal(rec.fidelity.expert, w["record"].expert)  # ... and reports the routes as launched
    _check_record(rec, w["want"], "case 1")
    _check_tables(tables, w["want"], "case 1")  # the device tables, in place, equal the host rule's
    assert rec.routes is tables
    state = w["want"].state_of_head.tolist()
    for h in range(H):
        if state[h] == 2:  # what routed_attention(fp8=False) writes for it under expert 0
            assert torch.equal(out[0, h], w["dense"][0, h]), f"repaired head {h}"
            assert not torch.equal(out[0, h], w["today"][0, h])
        else:  # a kept head keeps its bits
            assert torch.equal(out[0, h], w["today"][0, h]), f"kept head {h}"
    # a second call on the same tensors and the repaired tables repairs nothing and gives the same out
    out2, rec2 = routed_attention_repaired(c["q"], c["k"], c["v"], tables, c["geom"], repair_above=w["bound"], rows=c["rows"],
                                           model="wan", out=torch.zeros_like(c["q"]))
    assert int(rec2.repair_count) == 0 and 2 not in rec2.state_of_head.tolist()
    assert rec2.state_of_head.tolist() == [0 if s == 2 else s for s in state]  # (a repaired head's launch is the reference now)
    _check_tables(tables, w["want"], "case 1, second call")
    assert torch.equal(out2, out)


def test_single_native_tier_with_sparse_experts_and_text_rows():
    from vorta_amd.routed import routed_attention_repaired
    c = _case()
    hy = c["hunyuan"]
    routing, ids = _single_tables(c["dev"])
    out, rec = routed_attention_repaired(hy["q"], hy["k"], hy["v"], (routing, ids), c["geom"], repair_above=hy["bound"],
                                         rows=c["rows"], out=torch.zeros_like(hy["q"]), fp8=False, **hy["kw"])
    torch.cuda.synchronize()
    assert _same_record(rec.fidelity, hy["record"])
    _check_record(rec, hy["want"], "case 2")
    _check_tables(rec.routes, hy["want"], "case 2")
    # in place: the HeadRouting the caller holds reads the repaired lists and counts
    assert routing.counts_dev.tolist() == hy["want"].counts[0].tolist() and ids.tolist() == hy["want"].expert_of_head.tolist()
    state = hy["want"].state_of_head.tolist()
    S = c["geom"].S
    for h in range(H):
        if state[h] == 2:
            assert torch.equal(out[0, h, :S], hy["dense"][0, h, :S]), f"repaired head {h}: video rows"
            assert torch.equal(out[0, h, S:], hy["dense"][0, h, S:]), f"repaired head {h}: text rows"
        else:
            assert torch.equal(out[0, h], hy["today"][0, h]), f"kept head {h}"
    out2, rec2 = routed_attention_repaired(hy["q"], hy["k"], hy["v"], (routing, ids), c["geom"], repair_above=hy["bound"],
                                           rows=c["rows"], out=torch.zeros_like(hy["q"]), fp8=False, **hy["kw"])
    assert int(rec2.repair_count) == 0 and torch.equal(out2, out)


def test_the_whole_call_is_free_of_host_reads_and_a_captured_graph_follows_its_inputs():
    from vorta_amd.patch import repair_routes
    from vorta_amd.routed import routed_attention_repaired, routed_attention_tiers
    c = _case()
    w, dev, geom, rows = c["wan"], c["dev"], c["geom"], c["rows"]
    fresh = _tier_tables(dev)
    tables = _tier_tables(dev)
    q, k, v = (x.clone() for x in (c["q"], c["k"], c["v"]))
    out = torch.zeros_like(q)
    call = lambda: routed_attention_repaired(q, k, v, tables, geom, repair_above=w["bound"], rows=rows, model="wan", out=out)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on a side stream, as torch.cuda.graph asks
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for name in ("expert_ids", "tier_index", "lists", "counts"):
        getattr(tables, name).copy_(getattr(fresh, name))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # any host <-> device synchronisation in here raises
    try:
        _, rec = call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _check_record(rec, w["want"], "eager under sync debug")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, rec = call()
    # other inputs, whose violators differ: the heads rolled by one
    q2, k2, v2 = (x.roll(1, dims=1).contiguous() for x in (c["q"], c["k"], c["v"]))
    sink = []
    today2 = routed_attention_tiers(q2, k2, v2, fresh.routings, geom, model="wan", out=torch.zeros_like(q2), fidelity=sink,
                                    fidelity_rows=rows, fidelity_heads="all")
    want2 = repair_routes([0] * H, [0] * H, 2, 1, sink[0].sq_ref.cpu(), sink[0].sq_err.cpu(), w["bound"])
    assert want2.state_of_head.tolist() != w["want"].state_of_head.tolist() and want2.repair_count >= 1
    for inputs, want, today in (((q2, k2, v2), want2, today2), ((c["q"], c["k"], c["v"]), w["want"], w["today"])):
        for dst, src in zip((q, k, v), inputs):
            dst.copy_(src)
        for name in ("expert_ids", "tier_index", "lists", "counts"):
            getattr(tables, name).copy_(getattr(fresh, name))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _check_record(rec, want, "replay")
        _check_tables(tables, want, "replay")
        for h, s in enumerate(want.state_of_head.tolist()):
            assert torch.equal(out[0, h], today[0, h]) == (s != 2), (h, s)


def test_without_a_bound_the_call_is_todays():
    from vorta_amd import ops
    from vorta_amd.routed import routed_attention, routed_attention_repaired, routed_attention_tiers
    c = _case()
    hy = c["hunyuan"]

    def launches(fn):
        record, timeline = [], ops.Timeline()
        ops.set_timeline(timeline)
        try:
            out = fn(record)
        finally:
            ops.set_timeline(None)
        torch.cuda.synchronize()
        return out, record, [r[:4] for r in timeline.records]

    def same_launches(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x.keys() == y.keys()
            for key in x:
                if key == "out":
                    continue
                if torch.is_tensor(x[key]):
                    assert x[key].shape == y[key].shape and x[key].dtype == y[key].dtype, key
                    # (the coreset's row lists are written per call, and only for the slots under a device count: the slots
                    # past it hold what the allocator left -- their values are not part of the launch)
                    assert key in ("q_rows", "kv_rows", "dup_rows") or torch.equal(x[key], y[key]), key
                elif hasattr(x[key], "__slots__"):  # (ops.I8Operands: tensors under slots)
                    assert all(torch.equal(getattr(x[key], s), getattr(y[key], s)) for s in x[key].__slots__), key
                else:
                    assert x[key] == y[key], key

    tables = _tier_tables(c["dev"])
    a = launches(lambda r: routed_attention_tiers(c["q"], c["k"], c["v"], tables.routings, c["geom"], model="wan",
                                                  out=torch.zeros_like(c["q"]), record=r))
    b = launches(lambda r: routed_attention_repaired(c["q"], c["k"], c["v"], tables, c["geom"], repair_above=None, model="wan",
                                                     out=torch.zeros_like(c["q"]), record=r))
    assert b[0][1] is None and torch.equal(a[0], b[0][0]) and a[2] == b[2]
    same_launches(a[1], b[1])
    assert tables.expert_ids.tolist() == [0] * H and tables.counts.tolist() == [[H, 0, 0], [0, 0, 0]]  # nothing was decided
    routing, ids = _single_tables(c["dev"])
    a = launches(lambda r: routed_attention(hy["q"], hy["k"], hy["v"], routing, c["geom"], out=torch.zeros_like(hy["q"]),
                                            record=r, **hy["kw"]))
    b = launches(lambda r: routed_attention_repaired(hy["q"], hy["k"], hy["v"], (routing, ids), c["geom"], repair_above=None,
                                                     out=torch.zeros_like(hy["q"]), record=r, **hy["kw"]))
    assert b[0][1] is None and torch.equal(a[0], b[0][0]) and a[2] == b[2]
    same_launches(a[1], b[1])
    assert "repair" not in [tag for tag, *_ in b[2]]


def test_refusals_are_by_name():
    import vorta_amd.routed as rt
    from vorta_amd.routed import HeadRouting, RepairableRoutes, routed_attention_repaired
    c = _case()
    dev = c["dev"]
    kw = dict(rows=c["rows"], model="wan")
    no_native = RepairableRoutes(("i8pv",), _i32([0] * H, dev), _i32([0] * H, dev), _tier_tables(dev).lists[:1].contiguous(),
                                 _i32([[H, 0, 0]], dev))
    with pytest.raises(ValueError, match="must include 'native'"):
        routed_attention_repaired(c["q"], c["k"], c["v"], no_native, c["geom"], repair_above=0.1, **kw)
    for precision in ("i8pv", "fp8pv", "auto8"):
        with pytest.raises(ValueError, match="must be tier routes"):
            routed_attention_repaired(c["q"], c["k"], c["v"], _single_tables(dev), c["geom"], repair_above=0.1, fp8=precision, **kw)
    before = rt.DEFAULT_FP8
    try:
        rt.set_attention_precision("auto8")  # ... and by the process precision, where the call names none
        with pytest.raises(ValueError, match="'auto8' is not a tier name"):
            routed_attention_repaired(c["q"], c["k"], c["v"], _single_tables(dev), c["geom"], repair_above=0.1, **kw)
    finally:
        rt.DEFAULT_FP8 = before
    for bad in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="repair_above"):
            routed_attention_repaired(c["q"], c["k"], c["v"], _tier_tables(dev), c["geom"], repair_above=bad, **kw)
    with pytest.raises(ValueError, match="device counts"):
        routed_attention_repaired(c["q"], c["k"], c["v"], (HeadRouting.from_expert_ids(SPARSE, dev), _i32(SPARSE, dev)), c["geom"],
                                  repair_above=0.1, **kw)
    with pytest.raises(ValueError, match="TierRoutes"):
        routed_attention_repaired(c["q"], c["k"], c["v"], {"native": _single_tables(dev)[0]}, c["geom"], repair_above=0.1, **kw)
